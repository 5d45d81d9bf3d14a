// Helpers shared by the encoder kernels (pn_grid_op.hip: the stand-alone hash-grid op; pn_nerf_forward.hip: SH forward + fused network;
// pn_encoder_grad.hip: SH dy_dx and backward).  gfx950 only.
#pragma once
#include "pn_common.h"

// Half(w * float(v)) as c10::Half computes it: the float product is rounded to float FIRST and then to half (two roundings).  Written
// naively, `(_Float16)(w * (float)v)` is fused by hipcc into v_fma_mixlo_f16, which rounds the exact product ONCE, straight to half — a
// different result whenever the float rounding lands on a half tie (tests/test_gpu_half.py caught it: isolated features one half ulp off the oracle).
// The empty asm keeps the float product a value of its own.
__device__ __forceinline__ _Float16 half_of_product(float w, _Float16 v) {
    float p = w * (float)v;
    asm volatile("" : "+v"(p));
    return (_Float16)p;
}
template <typename T>
__device__ __forceinline__ T rounded_product(float w, T v);
template <>
__device__ __forceinline__ float rounded_product<float>(float w, float v) { return w * v; }
template <>
__device__ __forceinline__ _Float16 rounded_product<_Float16>(float w, _Float16 v) { return half_of_product(w, v); }


// Real SH basis in the reference's sign convention (shencoder.cu:50-68); constants are the closed forms of its comments.
#define SH_C0 0.28209479177387814f   /* 1/(2 sqrt(pi)) */
#define SH_C1 0.48860251190291992f   /* sqrt(3)/(2 sqrt(pi)) */
#define SH_C2A 1.0925484305920792f   /* sqrt(15)/(2 sqrt(pi)) */
#define SH_C2B 0.94617469575755997f  /* 3 sqrt(5)/(4 sqrt(pi)) */
#define SH_C2C 0.31539156525251999f  /* sqrt(5)/(4 sqrt(pi)) */
#define SH_C2D 0.54627421529603959f  /* sqrt(15)/(4 sqrt(pi)) */
#define SH_C3A 0.59004358992664352f  /* sqrt(70)/(8 sqrt(pi)) */
#define SH_C3B 2.8906114426405538f   /* sqrt(105)/(2 sqrt(pi)) */
#define SH_C3C 0.45704579946446572f  /* sqrt(42)/(8 sqrt(pi)) */
#define SH_C3D 0.3731763325901154f   /* sqrt(7)/(4 sqrt(pi)) */
#define SH_C3E 1.4453057213202769f   /* sqrt(105)/(4 sqrt(pi)) */


// training-side launcher (pn_encoder_grad.hip) the SH forward entry point chains into when dy_dx is requested
int pn_sh_dy_dx_launch(const float* inputs, float* dy_dx, uint32_t B, uint32_t C, hipStream_t st);
