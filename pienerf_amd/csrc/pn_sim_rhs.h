// The device code shared by the simulator's right-hand-side stages: contact (pn_contact.hip), force fields (pn_fields.hip), self-contact
// (pn_selfcontact.hip) and, for the wave sum, kinematic pins (pn_pins.hip).  Every unit that includes it compiles with -ffp-contract=fast; one source
// for these lines is what makes a point's state and a kernel's sum the same bits in all of them (pn_sim_accel_rhs runs the sum on its own).
#pragma once
#include <hip/hip_runtime.h>

#include "pn_sim_ip.h"

// A point's position and velocity: pn_ip_row_acc over its 8 kernels, slots 0..7 one after the other, dof then dof_vel, fp64, not rounded to fp32.
// False on a kernel id out of range (never with the tables solver.py builds; keeps every read inside its buffer): x and v then hold a partial sum.
__device__ __forceinline__ bool pn_ip_state(int p, int n_k, const double* __restrict__ dof, const double* __restrict__ dof_vel, const int* __restrict__ topo,
                                            const double* __restrict__ Nx, double x[3], double v[3]) {
    x[0] = x[1] = x[2] = 0.0;
    v[0] = v[1] = v[2] = 0.0;
    for (int i = 0; i < 8; i++) {
        const int k = topo[p * 8 + i];   // n_IP <= 2^27
        if ((unsigned)k >= (unsigned)n_k) return false;
        const double* S = Nx + ((size_t)p * 8 + i) * 10;
        pn_ip_row_acc(dof + (size_t)k * 30, S, x[0], x[1], x[2]);
        pn_ip_row_acc(dof_vel + (size_t)k * 30, S, v[0], v[1], v[2]);
    }
    return true;
}

// 30 sums (basis x component) over a wave's lanes by the shuffle tree 32, 16 ... 1: lane 0 holds the totals.  The tree is the same on every device.
__device__ __forceinline__ void pn_wave_sum30(double acc[30]) {
#pragma unroll
    for (int i = 0; i < 30; i++) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc[i] += __shfl_down(acc[i], off);
    }
}

// fetch_a of the forms whose law ran in a launch before this one: a = accel[p]
struct PnAccelRead {
    const double* __restrict__ accel;
    __device__ __forceinline__ void operator()(int p, double a[3]) const {
        a[0] = accel[(size_t)p * 3]; a[1] = accel[(size_t)p * 3 + 1]; a[2] = accel[(size_t)p * 3 + 2];
    }
};

// rhs_out[kid] = rhs_in[kid] + sum over the kernel's run of rho dx^3 Nx_csr[e][b] a_p[c]: the body of a stage's per-kernel launch, one workgroup of
// THREADS threads (whole waves) per GMLS kernel `kid`, t = threadIdx.x, `on` uniform over the launch.  Thread t takes the entries t, t + THREADS, ...
// of the kernel's run (kernel_bg / kernel_cnt / buffer: the (point, slot) pairs, ascending) in ascending order and adds m Nx[point, slot, b] a[c] into
// 30 sums, a = fetch_a(p, a): the point's acceleration.  Each wave adds its lanes by pn_wave_sum30, lane 0 of each wave puts its totals into LDS, and
// the 30 threads that write add the waves in the order ((w0 + w1) + w2) + w3.  No atomics; the order is a function of the run alone.  A kernel none of
// whose points has a != 0, and so every kernel of a launch with `on` false, copies rhs_in's bits (g + 0.0 would turn a -0.0 into +0.0).
template <int THREADS, typename A>
__device__ __forceinline__ void pn_kernel_accel_term(int kid, int t, bool on, int n_IP, double dx3, const double* __restrict__ rho,
                                                     const int* __restrict__ kernel_bg, const int* __restrict__ kernel_cnt, const int* __restrict__ buffer,
                                                     const double* __restrict__ Nx_csr, const double* __restrict__ rhs_in, double* __restrict__ rhs_out,
                                                     A fetch_a) {
    static_assert(THREADS % 64 == 0, "whole waves");
    constexpr int WAVES = THREADS / 64;
    __shared__ double s_part[WAVES][30];
    const int bg = min(max(kernel_bg[kid], 0), 8 * n_IP), end = min(bg + max(kernel_cnt[kid], 0), 8 * n_IP);
    const double* g = rhs_in + (size_t)kid * 30;
    double* o = rhs_out + (size_t)kid * 30;
    double acc[30];
#pragma unroll
    for (int i = 0; i < 30; i++) acc[i] = 0.0;
    int hit = 0;
    if (on) {
        for (int e = bg + t; e < end; e += THREADS) {
            const int p = buffer[e] >> 3;
            if ((unsigned)p >= (unsigned)n_IP) continue;  // never with the tables solver.py builds; keeps every read inside its buffer
            double a[3];
            fetch_a(p, a);
            if (a[0] == 0.0 && a[1] == 0.0 && a[2] == 0.0) continue;  // the stage does not act on this point
            hit = 1;
            const double m = rho[p] * dx3;
            const double* N = Nx_csr + (size_t)e * 10;
#pragma unroll
            for (int b = 0; b < 10; b++) {
                const double w = m * N[b];
#pragma unroll
                for (int c = 0; c < 3; c++) acc[b * 3 + c] += w * a[c];
            }
        }
    }
    if (!__syncthreads_or(hit)) {  // uniform over the workgroup
        if (t < 30) o[t] = g[t];
        return;
    }
    pn_wave_sum30(acc);
    if ((t & 63) == 0) {
#pragma unroll
        for (int i = 0; i < 30; i++) s_part[t >> 6][i] = acc[i];
    }
    __syncthreads();
    if (t < 30) {
        double s = s_part[0][t];
#pragma unroll
        for (int w = 1; w < WAVES; w++) s += s_part[w][t];
        o[t] = g[t] + s;
    }
}
