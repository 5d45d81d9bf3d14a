// Arbitrary rest-space points carried along by the simulator's GMLS field (simulator/binding.py: PointBinding.warp): the deforming surface mesh.
//
// The forward map is update_pos_kernel's (simulator/solver.py:604-617 of the reference), pos = sum_i sum_c Nx[p,i,c] dof[topo[p,i] 10 + c, :], for
// points that are not the sampling cloud's, plus the push-forward of a rest normal by the cofactor of the deformation gradient
// F[r][j] = sum_i sum_c dNx[p,i,j,c] dof[topo[p,i] 10 + c, r].
//
// Form: EIGHT LANES PER POINT, one per neighbour kernel (slot), eight points per wave.  The weight tables are stored per group of eight points in the
// order the lanes read them (include/pienerf_hip.h: pn_sim_warp_points), so every table load of a wave is one contiguous KiB, 16 bytes per lane; the
// dof rows (240 bytes per kernel, at most a few hundred kernels) come out of the caches.  Each lane forms its slot's share with pn_sim_ip.h's
// accumulation (c = 0..9 in order), then the eight shares are added in a fixed butterfly, ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7)): every lane
// of the point ends with the same bits, and they depend on nothing but the point's own row — not on its place in the group, the wave or the call.  No
// atomics, no scratch memory, no host synchronisation: one launch, legal inside a stream capture.
#include <math.h>

#include "pn_common.h"
#include "pn_sim_ip.h"

#define PN_WARP_GROUP 8      // points per wave = lanes per point
#define PN_WARP_THREADS 256  // four groups per workgroup

static_assert(PN_WARP_GROUP * 8 == PN_WAVE, "a group of points fills one wave, eight lanes per point");

// Sum over the 8 lanes of a point (lanes 8q .. 8q + 7), the same bits in all of them: IEEE addition is commutative, so both partners of an exchange
// compute the same sum.
__device__ __forceinline__ double pn_warp_sum8(double v) {
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 4);
    return v;
}

template <bool NORMALS>
__global__ void __launch_bounds__(PN_WARP_THREADS) k_warp_points(int n_pts, int n_k, const int* __restrict__ topo_g, const double2* __restrict__ Nx_g,
                                                                 const double2* __restrict__ dNx_g, const double* __restrict__ dof,
                                                                 const float* __restrict__ normals0, float* __restrict__ pos_out,
                                                                 float* __restrict__ normals_out) {
    const int lane = threadIdx.x % PN_WAVE;
    const size_t g = (size_t)blockIdx.x * (PN_WARP_THREADS / PN_WAVE) + threadIdx.x / PN_WAVE;   // group = wave
    if (g * PN_WARP_GROUP >= (size_t)n_pts) return;                                              // wave-uniform: the shuffles below see whole waves
    const size_t p = g * PN_WARP_GROUP + lane / 8;                                               // this lane's point; >= n_pts: a padding row (zero weights)
    const int slot = lane % 8;

    int kid = topo_g[g * PN_WAVE + lane];
    kid = (unsigned)kid < (unsigned)n_k ? kid : 0;   // the binding checks its topology; a foreign table must still not read outside dof
    double d[30];
    {
        const double2* __restrict__ dr = (const double2*)(dof + (size_t)kid * 30);   // 240-byte rows of a 16-byte aligned vector
#pragma unroll
        for (int x = 0; x < 15; x++) {
            const double2 v = dr[x];
            d[2 * x] = v.x;
            d[2 * x + 1] = v.y;
        }
    }
    double S[10];
#pragma unroll
    for (int x = 0; x < 5; x++) {
        const double2 v = Nx_g[(g * 5 + x) * PN_WAVE + lane];
        S[2 * x] = v.x;
        S[2 * x + 1] = v.y;
    }
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    pn_ip_row_acc(d, S, a0, a1, a2);
    a0 = pn_warp_sum8(a0);
    a1 = pn_warp_sum8(a1);
    a2 = pn_warp_sum8(a2);
    const bool writer = slot < 3 && p < (size_t)n_pts;   // lanes 0..2 of a point write its three components: 96 contiguous bytes per full wave
    if (writer) pos_out[p * 3 + slot] = (float)(slot == 0 ? a0 : (slot == 1 ? a1 : a2));

    if (NORMALS) {
        double F[3][3];   // F[r][j]
#pragma unroll
        for (int j = 0; j < 3; j++) {
#pragma unroll
            for (int x = 0; x < 5; x++) {
                const double2 v = dNx_g[(g * 15 + j * 5 + x) * PN_WAVE + lane];
                S[2 * x] = v.x;
                S[2 * x + 1] = v.y;
            }
            double f0 = 0.0, f1 = 0.0, f2 = 0.0;
            pn_ip_row_acc(d, S, f0, f1, f2);
            F[0][j] = pn_warp_sum8(f0);
            F[1][j] = pn_warp_sum8(f1);
            F[2][j] = pn_warp_sum8(f2);
        }
        if (writer) {
            const float m0 = normals0[p * 3], m1 = normals0[p * 3 + 1], m2 = normals0[p * 3 + 2];
            const double n0 = (double)m0, n1 = (double)m1, n2 = (double)m2;
            // cof(F) n = n0 (f1 x f2) + n1 (f2 x f0) + n2 (f0 x f1), f_j = column j of F: no division, no inverse
            double c[3];
#pragma unroll
            for (int r = 0; r < 3; r++) {
                const int r1 = (r + 1) % 3, r2 = (r + 2) % 3;
                const double x12 = F[r1][1] * F[r2][2] - F[r2][1] * F[r1][2];
                const double x20 = F[r1][2] * F[r2][0] - F[r2][2] * F[r1][0];
                const double x01 = F[r1][0] * F[r2][1] - F[r2][0] * F[r1][1];
                c[r] = n0 * x12 + n1 * x20 + n2 * x01;
            }
            const double len = sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
            const double cs = slot == 0 ? c[0] : (slot == 1 ? c[1] : c[2]);
            const float ms = slot == 0 ? m0 : (slot == 1 ? m1 : m2);
            normals_out[p * 3 + slot] = (len > 0.0 && isfinite(len)) ? (float)(cs / len) : ms;   // a collapsed or non-finite F keeps the rest normal
        }
    }
}

extern "C" int pn_sim_warp_points_group(void) { return PN_WARP_GROUP; }

extern "C" int pn_sim_warp_points(int n_pts, int n_k, const int* topo_g, const double* Nx_g, const double* dNx_g, const double* dof, const float* normals0,
                                  float* pos_out, float* normals_out, void* stream) {
    PN_REQUIRE(n_pts > 0 && n_k > 0 && topo_g && Nx_g && dof && pos_out);
    PN_REQUIRE(!normals_out || (dNx_g && normals0));
    PN_REQUIRE(((uintptr_t)Nx_g | (uintptr_t)dNx_g | (uintptr_t)dof) % 16 == 0);   // read 16 bytes per lane
    const uint32_t groups = pn_div_up((uint64_t)n_pts, PN_WARP_GROUP);
    const uint32_t blocks = pn_div_up(groups, PN_WARP_THREADS / PN_WAVE);
    hipStream_t s = (hipStream_t)stream;
    if (normals_out)
        k_warp_points<true><<<blocks, PN_WARP_THREADS, 0, s>>>(n_pts, n_k, topo_g, (const double2*)Nx_g, (const double2*)dNx_g, dof, normals0, pos_out,
                                                               normals_out);
    else
        k_warp_points<false><<<blocks, PN_WARP_THREADS, 0, s>>>(n_pts, n_k, topo_g, (const double2*)Nx_g, nullptr, dof, nullptr, pos_out, nullptr);
    PN_LAUNCH_CHECK();
    return PN_OK;
}
