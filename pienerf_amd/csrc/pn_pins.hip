// Kinematic pins: the pinned points of the cloud follow a scripted motion (include/pienerf_hip.h: pn_pin_motion).
//
// The system matrix holds stiff N N^T for every pinned point (build_pin_global, cuda_utils.py:58-81 of the reference), so a prescribed displacement
// u_p of pin p changes only the right-hand side, by stiff sum_p N_p^T u_p: the matrix and its inverse stay as they are, and so do the substep's
// kernels, which take the right-hand side's constant part as a plain pointer.  k_pin_rhs, enqueued in front of every substep, writes that part as
// rhs_ext = rhs_gravity + the pin term from a small state in device memory with its own substep clock, so a substep captured into a HIP graph — or
// run frames ahead of the render in the pipelined harness — gets the displacement of ITS OWN time; k_pin_tick behind it advances the clock.
#include <math.h>

#include "pn_common.h"
#include "pn_sim_rhs.h"

static_assert(sizeof(pn_pin_motion) == 128, "pn_pin_motion: 128 bytes (pienerf_amd/simulator/pins.py allocates it as 16 doubles)");

#define PN_PIN_THREADS 64   // one wave per GMLS kernel: the sum's tree is the wave's shuffle tree, fixed on every device
#define PN_2PI 6.283185307179586476925286766559

// ------------------------------------------------------------------------------------------------ the right-hand side, every substep
// One workgroup per GMLS kernel.  Lane l adds the run's entries l, l + 64, l + 128, ... in ascending order into 30 sums (basis x component), the
// lanes are added by pn_wave_sum30 (pn_sim_rhs.h: the shuffle tree 32, 16, ... 1), lane 0's total goes through LDS to the 30 lanes that write.  No atomics: the same bits on
// every run.  A kernel without an entry, or an inactive state, copies rhs_gravity (g + stiff 0 would turn a -0.0 into +0.0).
__global__ void __launch_bounds__(PN_PIN_THREADS) k_pin_rhs(int n_pin, const pn_pin_motion* __restrict__ st, double dt, double stiff,
                                                            const double* __restrict__ rhs_gravity, const int* __restrict__ pin_bg,
                                                            const int* __restrict__ pin_of, const double* __restrict__ pin_N,
                                                            const double* __restrict__ pin_X, const double* __restrict__ offsets,
                                                            double* __restrict__ rhs_ext) {
    __shared__ double s_sum[30];
    const int kid = blockIdx.x, lane = threadIdx.x;
    const int bg = max(pin_bg[kid], 0), end = min(pin_bg[kid + 1], 8 * n_pin);
    const double* g = rhs_gravity + (size_t)kid * 30;
    double* o = rhs_ext + (size_t)kid * 30;
    if (st->active == 0 || end <= bg) {  // uniform over the workgroup
        if (lane < 30) o[lane] = g[lane];
        return;
    }
    // the motion at the END of this implicit step.  (R - I) v = (n x v) sin a + (n (n.v) - v)(1 - cos a), 1 - cos a = 2 sin^2(a / 2): no cancellation
    // at small angles
    const double t = (double)(st->k + 1) * dt;
    const double sT = sin((PN_2PI * st->f_T) * t + st->phi_T);
    const double T0 = st->A[0] * sT, T1 = st->A[1] * sT, T2 = st->A[2] * sT;
    const double a = st->theta * sin((PN_2PI * st->f_R) * t + st->phi_R);
    const double sa = sin(a), sh = sin(0.5 * a), ca1 = 2.0 * sh * sh;
    const double n0 = st->n[0], n1 = st->n[1], n2 = st->n[2], c0 = st->c[0], c1 = st->c[1], c2 = st->c[2];
    double acc[30];
#pragma unroll
    for (int i = 0; i < 30; i++) acc[i] = 0.0;
    for (int e = bg + lane; e < end; e += PN_PIN_THREADS) {
        const int p = pin_of[e];
        if ((unsigned)p >= (unsigned)n_pin) continue;  // never with the tables solver.py builds; keeps every read inside its buffer
        const double v0 = pin_X[p * 3] - c0, v1 = pin_X[p * 3 + 1] - c1, v2 = pin_X[p * 3 + 2] - c2;
        const double nv = n0 * v0 + n1 * v1 + n2 * v2;
        double u[3];
        u[0] = T0 + (n1 * v2 - n2 * v1) * sa + (n0 * nv - v0) * ca1;
        u[1] = T1 + (n2 * v0 - n0 * v2) * sa + (n1 * nv - v1) * ca1;
        u[2] = T2 + (n0 * v1 - n1 * v0) * sa + (n2 * nv - v2) * ca1;
        if (offsets) {
            u[0] += offsets[p * 3]; u[1] += offsets[p * 3 + 1]; u[2] += offsets[p * 3 + 2];
        }
        const double* N = pin_N + (size_t)e * 10;
#pragma unroll
        for (int b = 0; b < 10; b++) {
            const double w = N[b];
#pragma unroll
            for (int c = 0; c < 3; c++) acc[b * 3 + c] += w * u[c];
        }
    }
    pn_wave_sum30(acc);
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 30; i++) s_sum[i] = acc[i];
    }
    __syncthreads();
    if (lane < 30) o[lane] = g[lane] + stiff * s_sum[lane];
}

// behind k_pin_rhs on the same stream: every workgroup of that launch has read the clock before it moves
__global__ void k_pin_tick(pn_pin_motion* __restrict__ st) { st->k += 1; }

extern "C" uint64_t pn_sim_pins_bytes(void) { return sizeof(pn_pin_motion); }

extern "C" int pn_sim_pins_rhs(int n_k, int n_pin, void* state, double dt, double stiff, const double* rhs_gravity, const int* pin_bg, const int* pin_of,
                               const double* pin_N, const double* pin_X, const double* offsets, double* rhs_ext, void* stream) {
    PN_REQUIRE(n_k > 0 && n_pin > 0 && n_pin <= (1 << 27) && state && rhs_gravity && pin_bg && pin_of && pin_N && pin_X && rhs_ext);
    PN_REQUIRE(isfinite(dt) && dt > 0.0 && isfinite(stiff));
    k_pin_rhs<<<n_k, PN_PIN_THREADS, 0, (hipStream_t)stream>>>(n_pin, (const pn_pin_motion*)state, dt, stiff, rhs_gravity, pin_bg, pin_of, pin_N, pin_X,
                                                                offsets, rhs_ext);
    PN_LAUNCH_CHECK();
    k_pin_tick<<<1, 1, 0, (hipStream_t)stream>>>((pn_pin_motion*)state);
    PN_LAUNCH_CHECK();
    return PN_OK;
}

// ------------------------------------------------------------------------------------------------ host-side updates
struct PnPinSet {
    int active, set_T, set_R;
    double T[5], R[9];
};

__global__ void k_pin_set(pn_pin_motion* __restrict__ st, PnPinSet s) {
    if (s.active >= 0) st->active = s.active;
    if (s.set_T) {
        for (int i = 0; i < 3; i++) st->A[i] = s.T[i];
        st->f_T = s.T[3]; st->phi_T = s.T[4];
    }
    if (s.set_R) {
        for (int i = 0; i < 3; i++) { st->n[i] = s.R[i]; st->c[i] = s.R[6 + i]; }
        st->theta = s.R[3]; st->f_R = s.R[4]; st->phi_R = s.R[5];
    }
}

extern "C" int pn_sim_pins_set(void* state, int n_pin, int active, const double* translate5_host, const double* rotate9_host, void* stream) {
    PN_REQUIRE(state && n_pin > 0 && active >= -1 && active <= 1);
    PnPinSet s;
    s.active = active; s.set_T = translate5_host != nullptr; s.set_R = rotate9_host != nullptr;
    for (int i = 0; i < 5; i++) {
        s.T[i] = translate5_host ? translate5_host[i] : 0.0;
        PN_REQUIRE(isfinite(s.T[i]));
    }
    for (int i = 0; i < 9; i++) {
        s.R[i] = rotate9_host ? rotate9_host[i] : 0.0;
        PN_REQUIRE(isfinite(s.R[i]));
    }
    if (rotate9_host && s.R[3] != 0.0) PN_REQUIRE(fabs(s.R[0] * s.R[0] + s.R[1] * s.R[1] + s.R[2] * s.R[2] - 1.0) <= 1e-9);  // a unit axis
    k_pin_set<<<1, 1, 0, (hipStream_t)stream>>>((pn_pin_motion*)state, s);
    PN_LAUNCH_CHECK();
    return PN_OK;
}

__global__ void k_pin_clock(pn_pin_motion* __restrict__ st, int64_t k) { st->k = k; }

extern "C" int pn_sim_pins_clock(void* state, int64_t k, void* stream) {
    PN_REQUIRE(state && k >= 0);
    k_pin_clock<<<1, 1, 0, (hipStream_t)stream>>>((pn_pin_motion*)state, k);
    PN_LAUNCH_CHECK();
    return PN_OK;
}
