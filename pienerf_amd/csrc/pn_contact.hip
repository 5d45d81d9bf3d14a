// Contact with planes, spheres, boxes and capsules (include/pienerf_hip.h: pn_contact_state).
//
// Ainv is pre-inverted, so contact is an explicit penalty on the right-hand side, scaled by m / dt^2 so that a point's own response to it is at most
// (kappa + beta) times its penetration.  The force depends on the integration points' current positions and velocities, so — the drag's argument
// (pn_drag.hip) — it is evaluated on the device: k_contact_points and k_contact_rhs, enqueued in front of every substep, write rhs_out = rhs_in + the
// contact term from a small state in device memory (parameters, 8 collider slots) and the dof / dof_vel that substep starts from.  A substep captured into a HIP graph,
// or run frames ahead of the render in the pipelined harness, gets the contact force of ITS OWN state, and a collider moved by the host between two
// replays is followed without a recapture.
#include <math.h>

#include "pn_common.h"
#include "pn_contact_law.h"
#include "pn_sdf.h"
#include "pn_sim_rhs.h"

static_assert(sizeof(pn_contact_collider) == 88, "pn_contact_collider: 88 bytes (pienerf_amd/simulator/contact.py: CONTACT_COLLIDER_DTYPE)");
static_assert(sizeof(pn_contact_state) == 744, "pn_contact_state: 744 bytes (pienerf_amd/simulator/contact.py: CONTACT_STATE_DTYPE)");
static_assert(PN_CONTACT_SLOTS == 8, "pn_contact_state: 8 collider slots");

#define PN_CONTACT_THREADS 256   // four waves per GMLS kernel; fixed: the order of the sum must not depend on the device

// ------------------------------------------------------------------------------------------------ the law, per integration point
// a += a_n n - a_t w_t / |w_t| over the colliders 0 .. n-1 in index order; returns whether any collider is penetrated (delta > 0).  A collider with
// delta = 0 adds exactly nothing.
__device__ __forceinline__ bool pn_contact_law(const pn_contact_state* __restrict__ st, int n, double dt, const double x[3], const double v[3], double a[3]) {
    const double kappa = st->kappa, beta = st->beta, mu = st->mu, h = st->h, dt2 = dt * dt;
    bool hit = false;
    a[0] = a[1] = a[2] = 0.0;
    for (int c = 0; c < n; c++) {   // one collider's part: pn_contact_law.h, shared with the rigid balls (pn_bodies.hip)
        double delta;
        if (pn_contact_collider_term(st->c + c, kappa, beta, mu, h, dt, dt2, x, v, a, &delta)) hit = true;
    }
    return hit;
}

// A point's position and velocity (pn_ip_state), then the law.  Returns whether the point is in contact; a = 0 when it is not.
__device__ __forceinline__ bool pn_contact_point(int p, int n_k, const pn_contact_state* __restrict__ st, int n, double dt, const double* __restrict__ dof,
                                                 const double* __restrict__ dof_vel, const int* __restrict__ topo, const double* __restrict__ Nx, double a[3]) {
    double x[3], v[3];
    a[0] = a[1] = a[2] = 0.0;
    if (!pn_ip_state(p, n_k, dof, dof_vel, topo, Nx, x, v)) return false;
    if (pn_contact_law(st, n, dt, x, v, a)) return true;
    a[0] = a[1] = a[2] = 0.0;
    return false;
}

// ------------------------------------------------------------------------------------------------ the law at every point (first of two launches)
// One thread per integration point: accel[p] = a_p, zeros for a point not in contact and for every point of an inactive or empty state.
#define PN_CONTACT_POINT_THREADS 64   // 3 576 points on the chair: 56 workgroups of one wave, spread over the CUs
__global__ void __launch_bounds__(PN_CONTACT_POINT_THREADS) k_contact_points(int n_k, int n_IP, const pn_contact_state* __restrict__ st, double dt,
                                                                             const double* __restrict__ dof, const double* __restrict__ dof_vel,
                                                                             const int* __restrict__ topo, const double* __restrict__ Nx,
                                                                             double* __restrict__ accel) {
    const int p = blockIdx.x * PN_CONTACT_POINT_THREADS + threadIdx.x;
    if (p >= n_IP) return;
    const int n = min(st->n, PN_CONTACT_SLOTS);
    double a[3] = {0.0, 0.0, 0.0};
    if (st->active != 0 && n > 0) pn_contact_point(p, n_k, st, n, dt, dof, dof_vel, topo, Nx, a);
    accel[(size_t)p * 3] = a[0]; accel[(size_t)p * 3 + 1] = a[1]; accel[(size_t)p * 3 + 2] = a[2];
}

// ------------------------------------------------------------------------------------------------ the right-hand side, every substep
// rhs_out = rhs_in + the contact term: pn_kernel_accel_term (pn_sim_rhs.h), one workgroup of four waves per GMLS kernel.  a = the point's contact
// acceleration: read from `accel` (written by k_contact_points in the launch before this one), or with FUSED evaluated here by the same
// pn_contact_point — 8 x redundant across a point's kernels, but one launch; every workgroup that evaluates a point runs the same code on the same
// inputs, so all agree on it to the bit.  A point not in contact has a = 0 (a penetrated collider always pushes: a_n > 0).
template <bool FUSED>
__global__ void __launch_bounds__(PN_CONTACT_THREADS) k_contact_rhs(int n_k, int n_IP, const pn_contact_state* __restrict__ st, double dt, double dx3,
                                                                    const double* __restrict__ dof, const double* __restrict__ dof_vel,
                                                                    const int* __restrict__ topo, const double* __restrict__ rho,
                                                                    const double* __restrict__ Nx, const int* __restrict__ kernel_bg,
                                                                    const int* __restrict__ kernel_cnt, const int* __restrict__ buffer,
                                                                    const double* __restrict__ Nx_csr, const double* __restrict__ rhs_in,
                                                                    double* __restrict__ rhs_out, const double* __restrict__ accel) {
    if (FUSED) {
        const int n = min(st->n, PN_CONTACT_SLOTS);
        const bool on = st->active != 0 && n > 0;  // uniform over the launch
        pn_kernel_accel_term<PN_CONTACT_THREADS>(blockIdx.x, threadIdx.x, on, n_IP, dx3, rho, kernel_bg, kernel_cnt, buffer, Nx_csr, rhs_in, rhs_out,
                                                 [&](int p, double a[3]) { pn_contact_point(p, n_k, st, n, dt, dof, dof_vel, topo, Nx, a); });
    } else {
        pn_kernel_accel_term<PN_CONTACT_THREADS>(blockIdx.x, threadIdx.x, true, n_IP, dx3, rho, kernel_bg, kernel_cnt, buffer, Nx_csr, rhs_in, rhs_out,
                                                 PnAccelRead{accel});
    }
}

// the shared sum on its own, `accel` as given: what the three stages' last launches compute (tests/test_gpu_rhs_term.py)
__global__ void __launch_bounds__(PN_CONTACT_THREADS) k_accel_rhs(int n_IP, double dx3, const double* __restrict__ rho, const int* __restrict__ kernel_bg,
                                                                  const int* __restrict__ kernel_cnt, const int* __restrict__ buffer,
                                                                  const double* __restrict__ Nx_csr, const double* __restrict__ rhs_in,
                                                                  double* __restrict__ rhs_out, const double* __restrict__ accel) {
    pn_kernel_accel_term<PN_CONTACT_THREADS>(blockIdx.x, threadIdx.x, true, n_IP, dx3, rho, kernel_bg, kernel_cnt, buffer, Nx_csr, rhs_in, rhs_out,
                                             PnAccelRead{accel});
}

extern "C" int pn_sim_accel_rhs(int n_k, int n_IP, double dx, const double* rho, const int* kernel_bg, const int* kernel_cnt, const int* buffer,
                                const double* Nx_csr, const double* accel, const double* rhs_in, double* rhs_out, void* stream) {
    PN_REQUIRE(n_k > 0 && n_IP > 0 && n_IP <= (1 << 27) && rho && kernel_bg && kernel_cnt && buffer && Nx_csr && accel);
    PN_REQUIRE(rhs_in && rhs_out && rhs_in != rhs_out);
    PN_REQUIRE(isfinite(dx) && dx > 0.0);
    k_accel_rhs<<<n_k, PN_CONTACT_THREADS, 0, (hipStream_t)stream>>>(n_IP, pow(dx, 3.0), rho, kernel_bg, kernel_cnt, buffer, Nx_csr, rhs_in, rhs_out, accel);
    PN_LAUNCH_CHECK();
    return PN_OK;
}

extern "C" uint64_t pn_sim_contact_bytes(void) { return sizeof(pn_contact_state); }

extern "C" int pn_sim_contact_rhs(int n_k, int n_IP, const void* state, double dt, double dx, const double* dof, const double* dof_vel, const int* topo,
                                  const double* rho, const double* Nx, const int* kernel_bg, const int* kernel_cnt, const int* buffer,
                                  const double* Nx_csr, const double* rhs_in, double* rhs_out, double* accel_out, void* stream) {
    PN_REQUIRE(n_k > 0 && n_IP > 0 && n_IP <= (1 << 27) && state && dof && dof_vel && topo && rho && Nx && kernel_bg && kernel_cnt && buffer && Nx_csr);
    PN_REQUIRE(rhs_in && rhs_out && rhs_in != rhs_out);
    PN_REQUIRE(isfinite(dt) && dt > 0.0 && isfinite(dx) && dx > 0.0);
    const pn_contact_state* st = (const pn_contact_state*)state;
    const double dx3 = pow(dx, 3.0);
    hipStream_t s = (hipStream_t)stream;
    if (accel_out) {  // two launches, the measured faster form: the law once per point, then the per-kernel sums
        k_contact_points<<<pn_div_up(n_IP, PN_CONTACT_POINT_THREADS), PN_CONTACT_POINT_THREADS, 0, s>>>(n_k, n_IP, st, dt, dof, dof_vel, topo, Nx, accel_out);
        PN_LAUNCH_CHECK();
        k_contact_rhs<false><<<n_k, PN_CONTACT_THREADS, 0, s>>>(n_k, n_IP, st, dt, dx3, dof, dof_vel, topo, rho, Nx, kernel_bg, kernel_cnt, buffer, Nx_csr,
                                                                 rhs_in, rhs_out, accel_out);
    } else {  // one launch: every entry evaluates its point itself
        k_contact_rhs<true><<<n_k, PN_CONTACT_THREADS, 0, s>>>(n_k, n_IP, st, dt, dx3, dof, dof_vel, topo, rho, Nx, kernel_bg, kernel_cnt, buffer, Nx_csr,
                                                                rhs_in, rhs_out, nullptr);
    }
    PN_LAUNCH_CHECK();
    return PN_OK;
}

// The two-launch form with the signed-distance grids' terms added between its launches (pn_sdf.hip: k_sdf_points): three launches.  The first and the
// last are pn_sim_contact_rhs's own kernels, so an empty sdf_state leaves its bits.
extern "C" int pn_sim_contact_sdf_rhs(int n_k, int n_IP, const void* state, const void* sdf_state, double dt, double dx, const double* dof,
                                      const double* dof_vel, const int* topo, const double* rho, const double* Nx, const int* kernel_bg,
                                      const int* kernel_cnt, const int* buffer, const double* Nx_csr, const double* rhs_in, double* rhs_out,
                                      double* accel_out, void* stream) {
    PN_REQUIRE(n_k > 0 && n_IP > 0 && n_IP <= (1 << 27) && state && sdf_state && dof && dof_vel && topo && rho && Nx && kernel_bg && kernel_cnt && buffer && Nx_csr);
    PN_REQUIRE(rhs_in && rhs_out && rhs_in != rhs_out && accel_out);
    PN_REQUIRE(isfinite(dt) && dt > 0.0 && isfinite(dx) && dx > 0.0);
    const pn_contact_state* st = (const pn_contact_state*)state;
    hipStream_t s = (hipStream_t)stream;
    k_contact_points<<<pn_div_up(n_IP, PN_CONTACT_POINT_THREADS), PN_CONTACT_POINT_THREADS, 0, s>>>(n_k, n_IP, st, dt, dof, dof_vel, topo, Nx, accel_out);
    PN_LAUNCH_CHECK();
    if (const int rc = pn_sdf_points_launch(n_k, n_IP, st, (const pn_sdf_state*)sdf_state, dt, dof, dof_vel, topo, Nx, accel_out, s)) return rc;
    k_contact_rhs<false><<<n_k, PN_CONTACT_THREADS, 0, s>>>(n_k, n_IP, st, dt, pow(dx, 3.0), dof, dof_vel, topo, rho, Nx, kernel_bg, kernel_cnt, buffer, Nx_csr,
                                                             rhs_in, rhs_out, accel_out);
    PN_LAUNCH_CHECK();
    return PN_OK;
}

// ------------------------------------------------------------------------------------------------ host-side updates
struct PnContactParams {
    int active, set;
    double p[4];
};

__global__ void k_contact_params(pn_contact_state* __restrict__ st, PnContactParams s) {
    if (s.active >= 0) st->active = s.active;
    if (s.set) {
        st->kappa = s.p[0]; st->beta = s.p[1]; st->mu = s.p[2]; st->h = s.p[3];
    }
}

extern "C" int pn_sim_contact_set_params(void* state, int active, const double* params4_host, void* stream) {
    PN_REQUIRE(state && active >= -1 && active <= 1);
    PnContactParams s;
    s.active = active; s.set = params4_host != nullptr;
    for (int i = 0; i < 4; i++) {
        s.p[i] = params4_host ? params4_host[i] : 0.0;
        PN_REQUIRE(isfinite(s.p[i]));
    }
    if (params4_host) {  // dt^2 a_n <= (kappa + beta) delta: with these ranges no step pushes a point further out than it was in
        PN_REQUIRE(s.p[0] > 0.0 && s.p[0] <= 1.0);
        PN_REQUIRE(s.p[1] >= 0.0 && s.p[1] <= 1.0);
        PN_REQUIRE(s.p[2] >= 0.0 && s.p[3] >= 0.0);
    }
    k_contact_params<<<1, 1, 0, (hipStream_t)stream>>>((pn_contact_state*)state, s);
    PN_LAUNCH_CHECK();
    return PN_OK;
}

struct PnContactSlot {
    int index, type;
    double g[10];
};

// writes the slot, then n = 1 + the highest slot in use: the launch visits the slots 0 .. n-1 and skips the empty ones
__global__ void k_contact_collider(pn_contact_state* __restrict__ st, PnContactSlot s) {
    pn_contact_collider* c = st->c + s.index;
    c->type = s.type; c->reserved = 0;
    for (int i = 0; i < 3; i++) { c->p[i] = s.g[i]; c->n[i] = s.g[3 + i]; c->v[i] = s.g[7 + i]; }
    c->R = s.g[6];
    int n = 0;
    for (int i = 0; i < PN_CONTACT_SLOTS; i++)
        if (st->c[i].type != PN_CONTACT_EMPTY) n = i + 1;
    st->n = n;
}

extern "C" int pn_sim_contact_set_collider(void* state, int index, int type, const double* geom10_host, void* stream) {
    PN_REQUIRE(state && index >= 0 && index < PN_CONTACT_SLOTS && type >= PN_CONTACT_EMPTY && type <= PN_CONTACT_CAPSULE);
    PN_REQUIRE(type == PN_CONTACT_EMPTY || geom10_host);
    PnContactSlot s;
    s.index = index; s.type = type;
    for (int i = 0; i < 10; i++) {
        s.g[i] = (type != PN_CONTACT_EMPTY && geom10_host) ? geom10_host[i] : 0.0;
        PN_REQUIRE(isfinite(s.g[i]));
    }
    if (type == PN_CONTACT_PLANE) PN_REQUIRE(fabs(s.g[3] * s.g[3] + s.g[4] * s.g[4] + s.g[5] * s.g[5] - 1.0) <= 1e-9);  // a unit normal
    if (type == PN_CONTACT_SPHERE || type == PN_CONTACT_CONTAINER) PN_REQUIRE(s.g[6] > 0.0);
    if (type == PN_CONTACT_BOX) PN_REQUIRE(s.g[3] > 0.0 && s.g[4] > 0.0 && s.g[5] > 0.0 && s.g[6] == 0.0);  // half-extents; R is reserved
    if (type == PN_CONTACT_CAPSULE) PN_REQUIRE(s.g[3] * s.g[3] + s.g[4] * s.g[4] + s.g[5] * s.g[5] > 0.0 && s.g[6] > 0.0);  // B - A, radius
    k_contact_collider<<<1, 1, 0, (hipStream_t)stream>>>((pn_contact_state*)state, s);
    PN_LAUNCH_CHECK();
    return PN_OK;
}
