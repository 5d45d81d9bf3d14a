// Q-GMLS elastodynamics substep for gfx950 (fp64, like the reference: simulator/func_utils.py:9-18).
//
// Reference (paths relative to /root/reference): simulator/solver.py:541-602 (build_rhs, compute_momentum,
// stepforward), simulator/cuda_utils.py:83-151,206-233 (calc_elastic, collect_rhs_IP, update_F_kernel),
// simulator/func_utils.py:21-40 (volume_invariant_project).  `wp.svd3` (warp-lang 0.13.0, not vendored) is restated
// by its contract: U, V proper rotations, smallest singular value carries the sign of det F.
//
// MI355X mapping:
//   * the reference's (30 n_k)^2 fp64 matrices are kron(A, I3) (solver.py:493-496), so only A (10 n_k)^2 is stored and
//     X[n,3] = A RHS[n,3] is one wave per row with a DPP/shuffle reduction: 9x fewer HBM bytes than the dense product;
//   * collect_rhs runs in gather form over a per-kernel CSR list (one wave per kernel, fixed summation tree): no fp64
//     atomics, bit-reproducible run to run;
//   * calc_elastic uses 8 lanes per integration point (one per neighbour kernel) so the 1.9 KB/IP of dNx is read coalesced.
//
// The unit in the order it is included (every pn_sim_*.h below except pn_sim_ip.h belongs to this translation unit alone):
//   pn_sim_ip.h       per-point arithmetic shared with pn_drag.hip and pn_warp_points.hip
//   pn_sim_svd.h      M3, the two svd3 (converged Jacobi, McAdams), volume_invariant_project, ip_F_partial (a lane's share of F, the same source for every form), shfl_xor_d
//   pn_sim_stamps.h   PN_SIM_PRIO and the timing build (-DPN_SIM_STAMPS=1)
// here: k_update_F, k_matvec3 (every form's dense products) and, at the end, k_update_force, each with its op-level entry; between them the substep's forms:
//   pn_sim_csr.h      launches over per-kernel CSR lists (k_elastic, the gathers, pn_sim_stepforward), calc_elastic / collect_rhs at op level
//   pn_sim_cells.h    one launch per local/global iteration over kernel-grid cells (k_cells_elastic_gather, pn_sim_stepforward_cells)
//   pn_sim_pcg.h      the cell form with the global step as a block-sparse PCG solve instead of the dense product (k_bsr_matvec3, k_pcg_*, pn_sim_stepforward_cells_pcg)
//   pn_sim_coop.h     all iterations in one persistent kernel (k_substep_coop, pn_sim_stepforward_coop)
#include <math.h>

#include "pn_common.h"
#include "pn_sim_ip.h"
#include "pn_sim_svd.h"
#include "pn_sim_stamps.h"

// ------------------------------------------------------------------------------------------------ update_F / get_IP_info
// One thread per (IP, shape-function row): row 0 = Nx -> pos; rows 1..3 = dNx[c] -> F[:,c]; rows 4..12 = ddNx[j][c] -> dF[j][:,c].
// Output already in get_IP_info's permuted fp32 layout (solver.py:422-424).
__global__ void __launch_bounds__(256) k_update_F(int n_IP, const int* __restrict__ topo, const double* __restrict__ dof, const double* __restrict__ Nx,
                                                  const double* __restrict__ dNx, const double* __restrict__ ddNx, float* __restrict__ pos,
                                                  float* __restrict__ F, float* __restrict__ dF) {
    PN_SIM_STAMP(4);
    PN_SIM_PRIO();
    const int tid = threadIdx.x + blockIdx.x * blockDim.x;
    const int v = tid / 13, row = tid % 13;
    if (v >= n_IP) return;
    double a0 = 0, a1 = 0, a2 = 0;
    for (int i = 0; i < 8; i++) {
        const int kid = topo[v * 8 + i];
        const double* __restrict__ S;
        if (row == 0) S = Nx + ((size_t)v * 8 + i) * 10;
        else if (row < 4) S = dNx + (((size_t)v * 8 + i) * 3 + (row - 1)) * 10;
        else S = ddNx + (((size_t)v * 8 + i) * 9 + (row - 4)) * 10;
        pn_ip_row_acc(dof + (size_t)kid * 30, S, a0, a1, a2);
    }
    if (row == 0) {
        pos[v * 3] = (float)a0; pos[v * 3 + 1] = (float)a1; pos[v * 3 + 2] = (float)a2;
    } else if (row < 4) {
        const int c = row - 1;  // F[r][c] -> flat c*3 + r
        F[v * 9 + c * 3] = (float)a0; F[v * 9 + c * 3 + 1] = (float)a1; F[v * 9 + c * 3 + 2] = (float)a2;
    } else {
        const int j = (row - 4) / 3, c = (row - 4) % 3;  // dF[j][r][c] -> flat c*9 + r*3 + j
        dF[v * 27 + c * 9 + j] = (float)a0; dF[v * 27 + c * 9 + 3 + j] = (float)a1; dF[v * 27 + c * 9 + 6 + j] = (float)a2;
    }
}

extern "C" int pn_sim_update_F(int n_IP, const int* topo, const double* dof, const double* Nx, const double* dNx, const double* ddNx, float* pos,
                               float* F, float* dF, void* stream) {
    PN_REQUIRE(n_IP > 0 && topo && dof && Nx && dNx && ddNx && pos && F && dF);
    k_update_F<<<pn_div_up((uint64_t)n_IP * 13, 256), 256, 0, (hipStream_t)stream>>>(n_IP, topo, dof, Nx, dNx, ddNx, pos, F, dF);
    PN_LAUNCH_CHECK();
    return PN_OK;
}

// ------------------------------------------------------------------------------------------------ structured matvec
// Y[i,:] = sum_j A[i,j] X[j,:], one wave per row.  Epilogues: 0: Y = s ; 1: Y = s + add1 + add2 (momentum, solver.py:576) ;
// 2: Y = add1 + s (dof = dof_rest + x, solver.py:601).
// 3: mode 2 + the substep's epilogue vel = (Y - add2) / dt * 0.998 (add2 = dof_last; k_step_end, solver.py:602).  Xv != nullptr (mode 1, the momentum
// product of a substep): X is read as X + dt * Xv (dof_tilde = dof + dt * vel, solver.py:575) and the first n * 3 threads also copy X to `copy_out`
// (dof_last = dof.clone(), :597) — what k_step_begin did in a launch of its own.
__global__ void __launch_bounds__(256) k_matvec3(int n, const double* __restrict__ A, const double* __restrict__ X, double* __restrict__ Y, int mode,
                                                 const double* __restrict__ add1, const double* __restrict__ add2, const double* __restrict__ Xv = nullptr,
                                                 double dt = 0.0, double* __restrict__ copy_out = nullptr, double* __restrict__ vel_out = nullptr) {
    PN_SIM_STAMP(3);
    PN_SIM_PRIO();
    if (copy_out) {
        const int g = blockIdx.x * blockDim.x + threadIdx.x;   // (two rows per wave = 32 threads per row >= its 3 entries)
        if (g < n * 3) copy_out[g] = X[g];
    }
    // two rows per wave: each X[j,:] fetched once serves both, and the four-deep unroll keeps 20 loads in flight per lane
    const int i0 = (blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * 2;
    if (i0 >= n) return;
    const bool two = i0 + 1 < n;
    const int lane = threadIdx.x & 63;
    const double* __restrict__ a = A + (size_t)i0 * n;
    const double* __restrict__ b = A + (size_t)(two ? i0 + 1 : i0) * n;
    double s[6] = {0, 0, 0, 0, 0, 0};
    int j = lane;
    for (; j + 192 < n; j += 256) {
        double wa[4], wb[4], x[4][3];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int jj = j + 64 * u;
            wa[u] = a[jj]; wb[u] = b[jj];
            x[u][0] = X[jj * 3]; x[u][1] = X[jj * 3 + 1]; x[u][2] = X[jj * 3 + 2];
            if (Xv) { x[u][0] = x[u][0] + dt * Xv[jj * 3]; x[u][1] = x[u][1] + dt * Xv[jj * 3 + 1]; x[u][2] = x[u][2] + dt * Xv[jj * 3 + 2]; }
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            s[0] += wa[u] * x[u][0]; s[1] += wa[u] * x[u][1]; s[2] += wa[u] * x[u][2];
            s[3] += wb[u] * x[u][0]; s[4] += wb[u] * x[u][1]; s[5] += wb[u] * x[u][2];
        }
    }
    for (; j < n; j += 64) {
        const double wa = a[j], wb = b[j];
        double x0 = X[j * 3], x1 = X[j * 3 + 1], x2 = X[j * 3 + 2];
        if (Xv) { x0 = x0 + dt * Xv[j * 3]; x1 = x1 + dt * Xv[j * 3 + 1]; x2 = x2 + dt * Xv[j * 3 + 2]; }
        s[0] += wa * x0; s[1] += wa * x1; s[2] += wa * x2;
        s[3] += wb * x0; s[4] += wb * x1; s[5] += wb * x2;
    }
#pragma unroll
    for (int q = 0; q < 6; q++)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s[q] += shfl_xor_d(s[q], o);
    if (lane < (two ? 6 : 3)) {
        double v = 0.0;
#pragma unroll
        for (int q = 0; q < 6; q++) if (q == lane) v = s[q];
        const size_t o = (size_t)i0 * 3 + lane;
        if (mode == 1) v = v + add1[o] + add2[o];
        else if (mode >= 2) v = add1[o] + v;
        Y[o] = v;
        if (mode == 3) vel_out[o] = (v - add2[o]) / dt * 0.998;
    }
}

extern "C" int pn_sim_matvec3(int n, const double* A, const double* X, double* Y, void* stream) {
    PN_REQUIRE(n > 0 && A && X && Y);
    k_matvec3<<<pn_div_up(n, 8), 256, 0, (hipStream_t)stream>>>(n, A, X, Y, 0, nullptr, nullptr);
    PN_LAUNCH_CHECK();
    return PN_OK;
}

// ------------------------------------------------------------------------------------------------ the three forms of the substep
#include "pn_sim_csr.h"
#include "pn_sim_cells.h"
#include "pn_sim_pcg.h"
#include "pn_sim_coop.h"

// ------------------------------------------------------------------------------------------------ update_force
// Simulator.update_force (solver.py:578-588): dof_f = the pick force of IP `vid` spread over its 8 kernels' 10 coefficients, zero
// elsewhere.  ONE launch writes every entry of dof_f (the reference: zero_ + an 80-iteration loop of scalar ops), so the vector never
// exists in a cleared-but-not-yet-filled state between two launches; vid < 0 = clear_force (:590-593).  The caller enqueues it on the
// stream the substeps run on (Simulator.force_stream), which orders it between two substeps.
__global__ void __launch_bounds__(256) k_update_force(int n30, int vid, double fx, double fy, double fz, double dx3, const int* __restrict__ topo,
                                                      const double* __restrict__ rho, const double* __restrict__ Nx, double* __restrict__ dof_f) {
    const int o = threadIdx.x + blockIdx.x * blockDim.x;
    if (o >= n30) return;
    dof_f[o] = vid >= 0 ? pn_force_entry(o, vid, fx, fy, fz, dx3, topo, rho, Nx) : 0.0;
}

extern "C" int pn_sim_update_force(int n_k, int vid, const double* f3_host, double dx, const int* topo, const double* rho, const double* Nx,
                                   double* dof_f, void* stream) {
    PN_REQUIRE(n_k > 0 && dof_f && (vid < 0 || (f3_host && topo && rho && Nx)));
    const double fx = vid >= 0 ? f3_host[0] : 0.0, fy = vid >= 0 ? f3_host[1] : 0.0, fz = vid >= 0 ? f3_host[2] : 0.0;
    k_update_force<<<pn_div_up((uint64_t)n_k * 30, 256), 256, 0, (hipStream_t)stream>>>(n_k * 30, vid, fx, fy, fz, pow(dx, 3.0), topo, rho, Nx, dof_f);
    PN_LAUNCH_CHECK();
    return PN_OK;
}
