// Stand-alone ray-side ops that share no kernel with the frame driver (gfx950): sph_from_ray, near/far, get_rays, packbits, morton3D and the static
// march.  Built with -ffp-contract=off (see pn_march_math.h).  Reference citations (raymarching.cu, nerf/...) name files of the reference implementation.
#include <float.h>

#include "pn_march_static.h"
#include "pn_near_far.h"
#include "pn_ray_dir.h"
#include "pn_sph.h"

// ------------------------------------------------------------------------------------------------ sph_from_ray
// kernel_sph_from_ray, raymarching.cu:165-202; the arithmetic is pn_sph.h's, shared with the fused background kernel (pn_background.hip).
__global__ void __launch_bounds__(256) k_sph_from_ray(const float* __restrict__ rays_o, const float* __restrict__ rays_d, float radius, uint32_t N,
                                                      float* __restrict__ coords) {
    const uint32_t n = threadIdx.x + blockIdx.x * blockDim.x;
    if (n >= N) return;
    float u, v;
    pn_sph_coords(rays_o[n * 3], rays_o[n * 3 + 1], rays_o[n * 3 + 2], rays_d[n * 3], rays_d[n * 3 + 1], rays_d[n * 3 + 2], radius, u, v);
    coords[n * 2] = u;
    coords[n * 2 + 1] = v;
}

extern "C" int pn_sph_from_ray(const float* rays_o, const float* rays_d, float radius, uint32_t N, float* coords, void* stream) {
    if (N == 0) return PN_OK;
    PN_REQUIRE(rays_o && rays_d && coords);
    k_sph_from_ray<<<pn_div_up(N, 256), 256, 0, (hipStream_t)stream>>>(rays_o, rays_d, radius, N, coords);
    PN_LAUNCH_CHECK();
    return PN_OK;
}

// ------------------------------------------------------------------------------------------------ near/far
// kernel_near_far_from_aabb, raymarching.cu:91-159 (the arithmetic is pn_near_far.h's, shared with the frame prologue)
__global__ void __launch_bounds__(256) k_near_far(const float* __restrict__ rays_o, const float* __restrict__ rays_d, const float* __restrict__ aabb,
                                                  uint32_t N, float min_near, float* __restrict__ nears, float* __restrict__ fars,
                                                  float* __restrict__ rays_t) {
    const uint32_t n = threadIdx.x + blockIdx.x * blockDim.x;
    if (n >= N) return;
    float near, far;
    pn_near_far(aabb, rays_o[n * 3], rays_o[n * 3 + 1], rays_o[n * 3 + 2], rays_d[n * 3], rays_d[n * 3 + 1], rays_d[n * 3 + 2], min_near, near, far);  // pn_near_far.h, shared with the frame prologue
    nears[n] = near;
    fars[n] = far;
    if (rays_t) rays_t[n] = near;  // frame driver: rays_t = nears.clone() (renderer.py:829)
}

extern "C" int pn_near_far_from_aabb(const float* rays_o, const float* rays_d, const float* aabb, uint32_t N, float min_near, float* nears,
                                     float* fars, void* stream) {
    if (N == 0) return PN_OK;  // empty tensors have null data pointers
    PN_REQUIRE(rays_o && rays_d && aabb && nears && fars);
    k_near_far<<<pn_div_up(N, 256), 256, 0, (hipStream_t)stream>>>(rays_o, rays_d, aabb, N, min_near, nears, fars, nullptr);
    PN_LAUNCH_CHECK();
    return PN_OK;
}

// ------------------------------------------------------------------------------------------------ get_rays
// nerf/utils.py:54-138 (N = -1): pixel p -> (i = p%W + .5, j = p/W + .5).  pose: device pointer, row-major 4x4 cam2world
// (the reference's `poses` is a device tensor too, so no host round trip is needed).
__global__ void __launch_bounds__(256) k_get_rays(const float* __restrict__ pose, float fx, float fy, float cx, float cy, int HW, int W,
                                                  float* __restrict__ rays_o, float* __restrict__ rays_d) {
    const int p = threadIdx.x + blockIdx.x * blockDim.x;
    if (p >= HW) return;
    pn_pixel_ray(pose, fx, fy, cx, cy, p % W, p / W, rays_o + p * 3, rays_d + p * 3);  // pn_ray_dir.h, shared with the training batch
}

extern "C" int pn_get_rays(const float* pose, float fx, float fy, float cx, float cy, int H, int W, float* rays_o, float* rays_d, void* stream) {
    PN_REQUIRE(pose && rays_o && rays_d && H > 0 && W > 0);
    k_get_rays<<<pn_div_up((uint64_t)H * W, 256), 256, 0, (hipStream_t)stream>>>(pose, fx, fy, cx, cy, H * W, W, rays_o, rays_d);
    PN_LAUNCH_CHECK();
    return PN_OK;
}

// ------------------------------------------------------------------------------------------------ static (undeformed) inference ops
// SURVEY 8(f) rank 3, inference side: kernel_march_rays (raymarching.cu:703-810), kernel_packbits (:270-292), kernel_morton3D /
// kernel_morton3D_invert (:217-258).  Off the simulate-and-render hot path (the deformed march of pn_render_ops.hip replaces kernel_march_rays
// there): one lane per ray / byte / index like the reference, arithmetic restated literally (this file is compiled with
// -ffp-contract=off) so that samples are bit-identical to the oracle.
__global__ void __launch_bounds__(128) k_march_rays_static(uint32_t n_alive, uint32_t n_step, const int* __restrict__ rays_alive,
                                                           const float* __restrict__ rays_t, const float* __restrict__ rays_o,
                                                           const float* __restrict__ rays_d, float bound, float dt_gamma, uint32_t max_steps, uint32_t C,
                                                           uint32_t H, const uint8_t* __restrict__ grid, const float* __restrict__ fars,
                                                           float* __restrict__ xyzs, float* __restrict__ dirs, float* __restrict__ deltas,
                                                           const float* __restrict__ noises) {
    const uint32_t n = threadIdx.x + blockIdx.x * blockDim.x;
    if (n >= n_alive) return;
    march_static_one<true, false>(n, n_step, rays_alive, rays_t, rays_o, rays_d, bound, dt_gamma, max_steps, C, H, grid, fars, xyzs, dirs, deltas, noises);  // pn_march_static.h
}

extern "C" int pn_march_rays(uint32_t n_alive, uint32_t n_step, const int* rays_alive, const float* rays_t, const float* rays_o, const float* rays_d,
                             float bound, float dt_gamma, uint32_t max_steps, uint32_t C, uint32_t H, const uint8_t* grid, const float* nears,
                             const float* fars, float* xyzs, float* dirs, float* deltas, const float* noises, void* stream) {
    (void)nears;
    if (n_alive == 0) return PN_OK;
    PN_REQUIRE(rays_alive && rays_t && rays_o && rays_d && grid && fars && xyzs && dirs && deltas);
    PN_REQUIRE(C >= 1 && C <= 8 && H > 0 && n_step >= 1 && max_steps > 0);
    k_march_rays_static<<<pn_div_up(n_alive, 128), 128, 0, (hipStream_t)stream>>>(n_alive, n_step, rays_alive, rays_t, rays_o, rays_d, bound, dt_gamma,
                                                                                 max_steps, C, H, grid, fars, xyzs, dirs, deltas, noises);
    PN_LAUNCH_CHECK();
    return PN_OK;
}

__global__ void __launch_bounds__(256) k_packbits(const float* __restrict__ grid, uint32_t N, float density_thresh, uint8_t* __restrict__ bitfield) {
    const uint32_t n = threadIdx.x + blockIdx.x * blockDim.x;
    if (n >= N) return;
    const float4 a = reinterpret_cast<const float4*>(grid)[2 * (size_t)n], b = reinterpret_cast<const float4*>(grid)[2 * (size_t)n + 1];
    const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    uint32_t bits = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) bits |= (v[i] > density_thresh) ? (1u << i) : 0u;
    bitfield[n] = (uint8_t)bits;
}

extern "C" int pn_packbits(const float* grid, uint32_t N, float density_thresh, uint8_t* bitfield, void* stream) {
    if (N == 0) return PN_OK;
    PN_REQUIRE(grid && bitfield && ((uintptr_t)grid & 15) == 0);
    k_packbits<<<pn_div_up(N, 256), 256, 0, (hipStream_t)stream>>>(grid, N, density_thresh, bitfield);
    PN_LAUNCH_CHECK();
    return PN_OK;
}

__device__ __forceinline__ uint32_t morton3D_invert1(uint32_t x) {  // raymarching.cu:73-81
    x = x & 0x49249249u;
    x = (x | (x >> 2)) & 0xc30c30c3u;
    x = (x | (x >> 4)) & 0x0f00f00fu;
    x = (x | (x >> 8)) & 0xff0000ffu;
    x = (x | (x >> 16)) & 0x0000ffffu;
    return x;
}
__global__ void __launch_bounds__(256) k_morton3D(const int* __restrict__ coords, uint32_t N, int* __restrict__ indices, int invert) {
    const uint32_t n = threadIdx.x + blockIdx.x * blockDim.x;
    if (n >= N) return;
    if (!invert) {
        indices[n] = (int)pnm::morton3D((uint32_t)coords[n * 3], (uint32_t)coords[n * 3 + 1], (uint32_t)coords[n * 3 + 2]);
    } else {  // `coords` is the output here
        const int ind = indices[n];
        int* c = const_cast<int*>(coords) + (size_t)n * 3;
        c[0] = (int)morton3D_invert1((uint32_t)(ind >> 0));
        c[1] = (int)morton3D_invert1((uint32_t)(ind >> 1));
        c[2] = (int)morton3D_invert1((uint32_t)(ind >> 2));
    }
}

extern "C" int pn_morton3D(const int* coords, uint32_t N, int* indices, void* stream) {
    if (N == 0) return PN_OK;
    PN_REQUIRE(coords && indices);
    k_morton3D<<<pn_div_up(N, 256), 256, 0, (hipStream_t)stream>>>(coords, N, indices, 0);
    PN_LAUNCH_CHECK();
    return PN_OK;
}

extern "C" int pn_morton3D_invert(const int* indices, uint32_t N, int* coords, void* stream) {
    if (N == 0) return PN_OK;
    PN_REQUIRE(coords && indices);
    k_morton3D<<<pn_div_up(N, 256), 256, 0, (hipStream_t)stream>>>(coords, N, const_cast<int*>(indices), 1);
    PN_LAUNCH_CHECK();
    return PN_OK;
}
