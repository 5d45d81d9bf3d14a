// Training-side SH encoder kernels for gfx950 (off the simulate-and-render hot path): dy_dx and backward.  The hash grid's are in pn_grid_op.hip.
//
// Reference: shencoder/src/shencoder.cu:125-355 (dy_dx branch of kernel_sh), :358-383 (kernel_sh_backward).
#include "pn_encoders.h"
#include "pn_sh_bands.h"

namespace {

// d/dx, d/dy, d/dz of the 16 polynomials of sh16 (pn_nerf_forward.hip); shencoder.cu:125-355 tabulates the same derivatives
__device__ __forceinline__ void sh16_grad(float x, float y, float z, float* gx, float* gy, float* gz) {
    const float xy = x * y, xz = x * z, yz = y * z, x2 = x * x, y2 = y * y, z2 = z * z;
#pragma unroll
    for (int i = 0; i < 16; i++) gx[i] = gy[i] = gz[i] = 0.0f;
    gy[1] = -SH_C1; gz[2] = SH_C1; gx[3] = -SH_C1;
    gx[4] = SH_C2A * y; gy[4] = SH_C2A * x;
    gy[5] = -SH_C2A * z; gz[5] = -SH_C2A * y;
    gz[6] = 2.0f * SH_C2B * z;
    gx[7] = -SH_C2A * z; gz[7] = -SH_C2A * x;
    gx[8] = 2.0f * SH_C2D * x; gy[8] = -2.0f * SH_C2D * y;
    gx[9] = -6.0f * SH_C3A * xy; gy[9] = SH_C3A * (-3.0f * x2 + 3.0f * y2);
    gx[10] = SH_C3B * yz; gy[10] = SH_C3B * xz; gz[10] = SH_C3B * xy;
    gy[11] = SH_C3C * (1.0f - 5.0f * z2); gz[11] = -10.0f * SH_C3C * yz;
    gz[12] = SH_C3D * (15.0f * z2 - 3.0f);
    gx[13] = SH_C3C * (1.0f - 5.0f * z2); gz[13] = -10.0f * SH_C3C * xz;
    gx[14] = 2.0f * SH_C3E * xz; gy[14] = -2.0f * SH_C3E * yz; gz[14] = SH_C3E * (x2 - y2);
    gx[15] = SH_C3A * (-3.0f * x2 + 3.0f * y2); gy[15] = 6.0f * SH_C3A * xy;
}

__global__ void __launch_bounds__(256) k_sh_dy_dx(const float* __restrict__ inputs, float* __restrict__ dy_dx, uint32_t B, uint32_t C) {
    const uint32_t b = threadIdx.x + blockIdx.x * blockDim.x;
    if (b >= B) return;
    float g[3][16];
    const float x = inputs[(size_t)b * 3], y = inputs[(size_t)b * 3 + 1], z = inputs[(size_t)b * 3 + 2];
    sh16_grad(x, y, z, g[0], g[1], g[2]);
    const uint32_t C2 = C * C;
    for (uint32_t d = 0; d < 3; d++)
        for (uint32_t i = 0; i < (C2 < 16u ? C2 : 16u); i++) dy_dx[((size_t)b * 3 + d) * C2 + i] = g[d][i];
    if (C > 4) {  // degree 5-8 (shencoder.cu:125-355): bands 4.. by recurrence, straight into the three rows
        float* row = dy_dx + (size_t)b * 3 * C2;
        pnsh::high_bands(x, y, z, (int)C, nullptr, row, row + C2, row + 2 * C2);
    }
}

__global__ void __launch_bounds__(256) k_sh_backward(const float* __restrict__ grad, uint32_t B, uint32_t C, const float* __restrict__ dy_dx,
                                                     float* __restrict__ grad_inputs) {
    const uint32_t t = threadIdx.x + blockIdx.x * blockDim.x;
    const uint32_t b = t / 3;
    if (b >= B) return;
    const uint32_t d = t - b * 3, C2 = C * C;
    float acc = grad_inputs[t];  // `+=` like the reference (shencoder.cu:378); the wrapper passes zeros
    for (uint32_t ch = 0; ch < C2; ch++) acc += grad[(size_t)b * C2 + ch] * dy_dx[((size_t)b * 3 + d) * C2 + ch];
    grad_inputs[t] = acc;
}

}  // namespace

int pn_sh_dy_dx_launch(const float* inputs, float* dy_dx, uint32_t B, uint32_t C, hipStream_t st) {
    k_sh_dy_dx<<<pn_div_up(B, 256), 256, 0, st>>>(inputs, dy_dx, B, C);
    PN_LAUNCH_CHECK();
    return PN_OK;
}

extern "C" int pn_sh_encode_backward(const float* grad, const float* inputs, uint32_t B, uint32_t D, uint32_t C, const float* dy_dx, float* grad_inputs,
                                     void* stream) {
    (void)inputs;
    if (B == 0) return PN_OK;
    PN_REQUIRE(grad && dy_dx && grad_inputs && D == 3 && C >= 1 && C <= 8);
    k_sh_backward<<<pn_div_up((uint64_t)B * 3, 256), 256, 0, (hipStream_t)stream>>>(grad, B, C, dy_dx, grad_inputs);
    PN_LAUNCH_CHECK();
    return PN_OK;
}
