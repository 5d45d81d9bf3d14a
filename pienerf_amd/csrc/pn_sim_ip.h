// Per-integration-point arithmetic shared by the simulator's kernels (pn_sim.hip) and the drag kernels (pn_drag.hip).  Both units compile with
// -ffp-contract=fast; keeping one source for these lines keeps their results the same bits in both (get_IP_info()'s pos == the drag's p0, and
// update_force's dof_f == the drag's dof_f for the same force).
#pragma once
#include <hip/hip_runtime.h>

// One kernel's share of an IP's shape-function row: a += dof[kid] (10 x 3) . S (10), in this order.  k_update_F sums the 8 neighbour kernels
// one after the other with it (row 0 = Nx -> the IP's position).
__device__ __forceinline__ void pn_ip_row_acc(const double* __restrict__ d, const double* __restrict__ S, double& a0, double& a1, double& a2) {
#pragma unroll
    for (int x = 0; x < 10; x++) {
        const double s = S[x];
        a0 += d[x * 3] * s;
        a1 += d[x * 3 + 1] * s;
        a2 += d[x * 3 + 2] * s;
    }
}

// Entry o of dof_f [10 n_k, 3] for the pick force (fx, fy, fz) on IP `vid` (solver.py:578-588): rho dx^3 Nx f on the IP's 8 kernels, zero elsewhere.
__device__ __forceinline__ double pn_force_entry(int o, int vid, double fx, double fy, double fz, double dx3, const int* __restrict__ topo,
                                                 const double* __restrict__ rho, const double* __restrict__ Nx) {
    double v = 0.0;
    const int row = o / 3, r = o - row * 3, kid = row / 10, j = row - kid * 10;
    const double f = r == 0 ? fx : (r == 1 ? fy : fz);
    const double m = rho[vid] * dx3;
    // an IP's 8 neighbour kernels are distinct, so at most one slot matches; summing keeps the reference's `+=` semantics otherwise
    for (int i = 0; i < 8; i++)
        if (topo[vid * 8 + i] == kid) v += m * Nx[((size_t)vid * 8 + i) * 10 + j] * f;
    return v;
}
