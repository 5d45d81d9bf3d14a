// Force fields: wind, vortex and blast on the whole body, with air drag (include/pienerf_hip.h: pn_field_state).
//
// A body force depends on the position and the velocity of every integration point, so — the drag's and contact's argument (pn_drag.hip,
// pn_contact.hip) — it is evaluated on the device: k_field_points and k_field_rhs, enqueued in front of every substep, write rhs_out = rhs_in + the
// field term from a small state in device memory (8 field slots and a substep clock of its own) and the dof / dof_vel that substep starts from;
// k_field_tick behind them advances the clock.  A substep captured into a HIP graph, or run frames ahead of the render in the pipelined harness, gets
// the force of ITS OWN state and ITS OWN time, and a field changed by the host between two replays is followed without a recapture.  The matrix, Ainv
// and the substep's kernels stay as they are: the two clamps of the law keep a point's own response per step bounded by what drives it.
#include <math.h>

#include "pn_common.h"
#include "pn_sim_rhs.h"

static_assert(sizeof(pn_force_field) == 144, "pn_force_field: 144 bytes (pienerf_amd/simulator/fields.py: FIELD_DTYPE)");
static_assert(sizeof(pn_field_state) == 1168, "pn_field_state: 1168 bytes (pienerf_amd/simulator/fields.py: FIELD_STATE_DTYPE)");
static_assert(PN_FIELD_SLOTS == 8, "pn_field_state: 8 field slots");

#define PN_FIELD_THREADS 256   // four waves per GMLS kernel; fixed: the order of the sum must not depend on the device
#define PN_FIELD_2PI 6.283185307179586476925286766559

// ------------------------------------------------------------------------------------------------ the law, per integration point
__device__ __forceinline__ double pn_field_fall(double q, double R) {
    const double w = fmax(1.0 - q / R, 0.0);
    return w * w;
}

// a = the sum over the fields 0 .. n-1 in index order, each only while t0 <= t < t1; an empty slot, a closed window, a point at or beyond R and a point
// at a blast's centre add exactly nothing.
__device__ __forceinline__ void pn_field_law(const pn_field_state* __restrict__ st, int n, double t, double dt, const double x[3], const double v[3],
                                             double a[3]) {
    const double c_max = 1.0 / dt, dt2 = dt * dt;
    a[0] = a[1] = a[2] = 0.0;
    for (int i = 0; i < n; i++) {
        const pn_force_field* f = st->f + i;
        const int type = f->type;
        if (type < PN_FIELD_WIND || type > PN_FIELD_RADIAL) continue;
        if (!(f->t0 <= t && t < f->t1)) continue;
        const double r0 = x[0] - f->p[0], r1 = x[1] - f->p[1], r2 = x[2] - f->p[2];
        if (type == PN_FIELD_WIND) {
            const double c = fmin(f->c, c_max);
            const double kr = f->kv[0] * r0 + f->kv[1] * r1 + f->kv[2] * r2;
            const double gust = 1.0 + f->g * sin(PN_FIELD_2PI * (f->f * t - kr) + f->phi);
            a[0] += c * (f->n[0] * gust - v[0]);
            a[1] += c * (f->n[1] * gust - v[1]);
            a[2] += c * (f->n[2] * gust - v[2]);
        } else if (type == PN_FIELD_VORTEX) {
            const double n0 = f->n[0], n1 = f->n[1], n2 = f->n[2];
            const double nr = n0 * r0 + n1 * r1 + n2 * r2;
            const double q0 = r0 - nr * n0, q1 = r1 - nr * n1, q2 = r2 - nr * n2;
            const double w = pn_field_fall(sqrt(q0 * q0 + q1 * q1 + q2 * q2), f->R);
            if (!(w > 0.0)) continue;
            const double cw = fmin(f->c, c_max) * w, om = f->s;
            a[0] += cw * (om * (n1 * r2 - n2 * r1) - v[0]);
            a[1] += cw * (om * (n2 * r0 - n0 * r2) - v[1]);
            a[2] += cw * (om * (n0 * r1 - n1 * r0) - v[2]);
        } else {
            const double L = sqrt(r0 * r0 + r1 * r1 + r2 * r2);
            const double w = pn_field_fall(L, f->R);
            if (!(L > 0.0) || !(w > 0.0)) continue;
            const double s = copysign(fmin(fabs(f->s), f->R / (2.0 * dt2)), f->s) * w;
            a[0] += s * (r0 / L); a[1] += s * (r1 / L); a[2] += s * (r2 / L);
        }
    }
}

// ------------------------------------------------------------------------------------------------ the law at every point (first of three launches)
// One thread per integration point: its position and velocity (pn_ip_state), then the law at t = k dt: accel[p] = a_p, zeros for every point of an
// inactive or empty state.
#define PN_FIELD_POINT_THREADS 64   // 3 576 points on the chair: 56 workgroups of one wave, spread over the CUs
__global__ void __launch_bounds__(PN_FIELD_POINT_THREADS) k_field_points(int n_k, int n_IP, const pn_field_state* __restrict__ st, double dt,
                                                                         const double* __restrict__ dof, const double* __restrict__ dof_vel,
                                                                         const int* __restrict__ topo, const double* __restrict__ Nx,
                                                                         double* __restrict__ accel) {
    const int p = blockIdx.x * PN_FIELD_POINT_THREADS + threadIdx.x;
    if (p >= n_IP) return;
    const int n = min(max(st->n, 0), PN_FIELD_SLOTS);
    double a[3] = {0.0, 0.0, 0.0};
    if (st->active != 0 && n > 0) {
        double x[3], v[3];
        if (pn_ip_state(p, n_k, dof, dof_vel, topo, Nx, x, v)) pn_field_law(st, n, (double)st->k * dt, dt, x, v, a);
    }
    accel[(size_t)p * 3] = a[0]; accel[(size_t)p * 3 + 1] = a[1]; accel[(size_t)p * 3 + 2] = a[2];
}

// ------------------------------------------------------------------------------------------------ the right-hand side, every substep
// rhs_out = rhs_in + the field term: pn_kernel_accel_term (pn_sim_rhs.h), one workgroup of four waves per GMLS kernel, a read from `accel` (written
// by k_field_points in the launch before this one).  Every kernel of a state that is inactive, empty or outside all its windows copies rhs_in's bits.
__global__ void __launch_bounds__(PN_FIELD_THREADS) k_field_rhs(int n_IP, const pn_field_state* __restrict__ st, double dx3, const double* __restrict__ rho,
                                                                const int* __restrict__ kernel_bg, const int* __restrict__ kernel_cnt,
                                                                const int* __restrict__ buffer, const double* __restrict__ Nx_csr,
                                                                const double* __restrict__ rhs_in, double* __restrict__ rhs_out,
                                                                const double* __restrict__ accel) {
    const bool on = st->active != 0 && st->n > 0;  // uniform over the launch
    pn_kernel_accel_term<PN_FIELD_THREADS>(blockIdx.x, threadIdx.x, on, n_IP, dx3, rho, kernel_bg, kernel_cnt, buffer, Nx_csr, rhs_in, rhs_out,
                                           PnAccelRead{accel});
}

// behind k_field_points and k_field_rhs on the same stream: every thread that reads the clock has read it before it moves
__global__ void k_field_tick(pn_field_state* __restrict__ st) { st->k += 1; }

extern "C" uint64_t pn_sim_fields_bytes(void) { return sizeof(pn_field_state); }

extern "C" int pn_sim_fields_rhs(int n_k, int n_IP, void* state, double dt, double dx, const double* dof, const double* dof_vel, const int* topo,
                                 const double* rho, const double* Nx, const int* kernel_bg, const int* kernel_cnt, const int* buffer,
                                 const double* Nx_csr, const double* rhs_in, double* rhs_out, double* accel_out, void* stream) {
    PN_REQUIRE(n_k > 0 && n_IP > 0 && n_IP <= (1 << 27) && state && dof && dof_vel && topo && rho && Nx && kernel_bg && kernel_cnt && buffer && Nx_csr);
    PN_REQUIRE(rhs_in && rhs_out && rhs_in != rhs_out && accel_out);
    PN_REQUIRE(isfinite(dt) && dt > 0.0 && isfinite(dx) && dx > 0.0);
    pn_field_state* st = (pn_field_state*)state;
    const double dx3 = pow(dx, 3.0);
    hipStream_t s = (hipStream_t)stream;
    k_field_points<<<pn_div_up(n_IP, PN_FIELD_POINT_THREADS), PN_FIELD_POINT_THREADS, 0, s>>>(n_k, n_IP, st, dt, dof, dof_vel, topo, Nx, accel_out);
    PN_LAUNCH_CHECK();
    k_field_rhs<<<n_k, PN_FIELD_THREADS, 0, s>>>(n_IP, st, dx3, rho, kernel_bg, kernel_cnt, buffer, Nx_csr, rhs_in, rhs_out, accel_out);
    PN_LAUNCH_CHECK();
    k_field_tick<<<1, 1, 0, s>>>(st);
    PN_LAUNCH_CHECK();
    return PN_OK;
}

// ------------------------------------------------------------------------------------------------ host-side updates
__global__ void k_field_active(pn_field_state* __restrict__ st, int active) { st->active = active; }

extern "C" int pn_sim_fields_set_active(void* state, int active, void* stream) {
    PN_REQUIRE(state && (active == 0 || active == 1));
    k_field_active<<<1, 1, 0, (hipStream_t)stream>>>((pn_field_state*)state, active);
    PN_LAUNCH_CHECK();
    return PN_OK;
}

struct PnFieldSlot {
    int index, type;
    double g[17];
};

// writes the slot, then n = 1 + the highest slot in use: the launch visits the slots 0 .. n-1 and skips the empty ones
__global__ void k_field_slot(pn_field_state* __restrict__ st, PnFieldSlot s) {
    pn_force_field* f = st->f + s.index;
    f->type = s.type; f->reserved = 0;
    for (int i = 0; i < 3; i++) { f->p[i] = s.g[i]; f->n[i] = s.g[3 + i]; f->kv[i] = s.g[12 + i]; }
    f->c = s.g[6]; f->s = s.g[7]; f->R = s.g[8]; f->g = s.g[9]; f->f = s.g[10]; f->phi = s.g[11]; f->t0 = s.g[15]; f->t1 = s.g[16];
    int n = 0;
    for (int i = 0; i < PN_FIELD_SLOTS; i++)
        if (st->f[i].type != PN_FIELD_EMPTY) n = i + 1;
    st->n = n;
}

extern "C" int pn_sim_fields_set_field(void* state, int index, int type, const double* geom17_host, void* stream) {
    PN_REQUIRE(state && index >= 0 && index < PN_FIELD_SLOTS && type >= PN_FIELD_EMPTY && type <= PN_FIELD_RADIAL);
    PN_REQUIRE(type == PN_FIELD_EMPTY || geom17_host);
    PnFieldSlot s;
    s.index = index; s.type = type;
    for (int i = 0; i < 17; i++) {
        s.g[i] = (type != PN_FIELD_EMPTY && geom17_host) ? geom17_host[i] : 0.0;
        PN_REQUIRE(isfinite(s.g[i]) || (i == 16 && s.g[i] > 0.0 && isinf(s.g[i])));  // only t1 may be +inf
    }
    PN_REQUIRE(s.g[6] >= 0.0);                       // c
    PN_REQUIRE(s.g[9] >= 0.0 && s.g[9] <= 1.0);      // g
    PN_REQUIRE(s.g[16] >= s.g[15]);                  // t1 >= t0
    if (type == PN_FIELD_VORTEX || type == PN_FIELD_RADIAL) PN_REQUIRE(s.g[8] > 0.0);
    if (type == PN_FIELD_VORTEX) PN_REQUIRE(fabs(s.g[3] * s.g[3] + s.g[4] * s.g[4] + s.g[5] * s.g[5] - 1.0) <= 1e-9);  // a unit axis
    k_field_slot<<<1, 1, 0, (hipStream_t)stream>>>((pn_field_state*)state, s);
    PN_LAUNCH_CHECK();
    return PN_OK;
}

__global__ void k_field_clock(pn_field_state* __restrict__ st, int64_t k) { st->k = k; }

extern "C" int pn_sim_fields_clock(void* state, int64_t k, void* stream) {
    PN_REQUIRE(state && k >= 0);
    k_field_clock<<<1, 1, 0, (hipStream_t)stream>>>((pn_field_state*)state, k);
    PN_LAUNCH_CHECK();
    return PN_OK;
}
