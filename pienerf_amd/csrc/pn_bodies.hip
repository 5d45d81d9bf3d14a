// Rigid balls: dynamic sphere colliders the object pushes back (include/pienerf_hip.h: pn_bodies_state has the law).
//
// A body's centre and velocity are its collider slot's p and v in the pn_contact_state, so contact (pn_contact.hip), the drawn frame and the shadows
// (pn_colliders.hip) follow a moving ball as they are.  What this unit adds is the reaction on the ball and its integration, as two launches behind
// contact's in front of every substep: both read the state the substep starts from, and — the argument of drag, pins, contact and the fields — a
// substep captured into a HIP graph, or run frames ahead of the render, moves the ball from ITS OWN state.
#include <math.h>

#include "pn_common.h"
#include "pn_contact_law.h"
#include "pn_sim_rhs.h"

static_assert(sizeof(pn_body) == 72, "pn_body: 72 bytes (pienerf_amd/simulator/bodies.py: BODY_DTYPE)");
static_assert(sizeof(pn_bodies_state) == 616, "pn_bodies_state: 616 bytes (pienerf_amd/simulator/bodies.py: BODIES_STATE_DTYPE)");
static_assert(PN_BODIES_SLOTS == PN_CONTACT_SLOTS, "body b lives in collider slot b");

#define PN_BODY_THREADS 256                   // fixed: the order of the sum must not depend on the device
#define PN_BODY_WAVES (PN_BODY_THREADS / 64)
#define PN_BODY_PART (PN_BODIES_SLOTS * 4)    // doubles per workgroup in `work`: (F[3], delta_max) per slot
#define PN_BODY_CS (sizeof(pn_contact_state) / 8)   // the two states as doubles: pn_body_step's copies in LDS
#define PN_BODY_BS (sizeof(pn_bodies_state) / 8)
#define PN_BODY_STEP_LDS (PN_BODY_PART + PN_BODY_CS + PN_BODY_BS)

// slot b moves by itself: marked dynamic, and the contact state holds a solid sphere there
__device__ __forceinline__ bool pn_body_dynamic(const pn_bodies_state* __restrict__ bs, const pn_contact_state* __restrict__ cs, int b) {
    return bs->b[b].dynamic != 0 && cs->c[b].type == PN_CONTACT_SPHERE;
}

// ------------------------------------------------------------------------------------------------ clamp, static colliders, integration
// The work of one workgroup of PN_BODY_THREADS threads, `lds` PN_BODY_STEP_LDS doubles.  The workgroup first copies the two states into LDS with one
// load per thread, so that what follows reads them at LDS latency and not through a chain of dependent global loads; the copies are what the step
// starts from, the stores go to the states themselves.  Thread t < 32 adds word t of the n_wg partials in ascending workgroup order (delta_max: the
// maximum; the loads of eight workgroups in flight at a time, the additions one after the other); then thread b < 8 does slot b.  A dynamic slot is
// written by its own thread alone (two dynamic balls do not see each other).
__device__ __forceinline__ void pn_body_step(int t, int n_wg, pn_bodies_state* gbs, pn_contact_state* gcs, double dt, const double* part, double* lds) {
    static_assert(PN_BODY_CS + PN_BODY_BS <= PN_BODY_THREADS, "one load per thread");
    double* s_tot = lds;
    if (t < (int)PN_BODY_CS) lds[PN_BODY_PART + t] = ((const double*)gcs)[t];
    else if (t < (int)(PN_BODY_CS + PN_BODY_BS)) lds[PN_BODY_PART + t] = ((const double*)gbs)[t - PN_BODY_CS];
    double s = 0.0;
    if (t < PN_BODY_PART) {
        if ((t & 3) == 3) {
#pragma unroll 8
            for (int w = 0; w < n_wg; w++) s = fmax(s, part[(size_t)w * PN_BODY_PART + t]);
        } else {
#pragma unroll 8
            for (int w = 0; w < n_wg; w++) s += part[(size_t)w * PN_BODY_PART + t];
        }
        s_tot[t] = s;
    }
    __syncthreads();
    const pn_contact_state* cs = (const pn_contact_state*)(lds + PN_BODY_PART);
    const pn_bodies_state* bs = (const pn_bodies_state*)(lds + PN_BODY_PART + PN_BODY_CS);
    const bool on = bs->active != 0 && cs->active != 0;
    const int n = min(cs->n, PN_CONTACT_SLOTS);
    const bool mine = on && t < PN_BODIES_SLOTS && t < n && pn_body_dynamic(bs, cs, t);
    double p[3] = {0.0, 0.0, 0.0}, u[3] = {0.0, 0.0, 0.0}, as[3] = {0.0, 0.0, 0.0};
    if (mine) {
        const pn_contact_collider* me = cs->c + t;
        const double R = me->R, kappa = cs->kappa, beta = cs->beta, mu = cs->mu;
        for (int i = 0; i < 3; i++) { p[i] = me->p[i]; u[i] = me->v[i]; }
        for (int c = 0; c < n; c++) {  // the static colliders, in index order: the law at the ball's centre, its radius as the thickness
            if (c == t || pn_body_dynamic(bs, cs, c)) continue;
            double delta;
            pn_contact_collider_term(cs->c + c, kappa, beta, mu, R, dt, dt * dt, p, u, as, &delta);
        }
    }
    if (mine) {
        pn_body* b = gbs->b + t;
        const double M = bs->b[t].M, F0 = 0.0 - s_tot[t * 4], F1 = 0.0 - s_tot[t * 4 + 1], F2 = 0.0 - s_tot[t * 4 + 2], dmax = s_tot[t * 4 + 3];
        const double Fn = sqrt(F0 * F0 + F1 * F1 + F2 * F2);
        double s = 1.0;
        if (Fn > 0.0) s = fmin(1.0, M * dmax / (dt * dt * Fn));
        if (s < 1.0) b->clamped = bs->b[t].clamped + 1;
        b->F[0] = F0; b->F[1] = F1; b->F[2] = F2; b->s = s; b->delta_max = dmax;
        const double F[3] = {F0, F1, F2}, den = 1.0 + dt * bs->b[t].c;
        pn_contact_collider* me = gcs->c + t;
        for (int i = 0; i < 3; i++) {
            const double un = (u[i] + dt * (bs->g[i] + s * F[i] / M + as[i])) / den;
            me->v[i] = un;
            me->p[i] = p[i] + dt * un;
        }
    }
    if (t == 0) gbs->k = bs->k + 1;
}

// ------------------------------------------------------------------------------------------------ the reaction's partial sums (first of two launches)
// One thread per integration point.  For every dynamic slot the point's m_i a_{i,b} and delta; the workgroup adds them by a wave's shuffle tree and
// then the waves in the order ((w0 + w1) + w2) + w3 through LDS, and threads 0 .. 31 write part[blockIdx.x][slot][F0, F1, F2, delta_max]: all 32
// words, zeros for a slot that is not dynamic or not touched (the sums start from +0.0).  The sign of F_b is pn_body_step's.
// ONE: the one-launch form.  Every workgroup publishes its partials (an agent-scope release in front of its ticket) and draws a ticket from the
// arrival counter behind them; the workgroup that draws the last one acquires, zeroes the counter for the next launch and runs pn_body_step itself:
// the same sums in the same order, so the same bits.  By then every other workgroup has read what the step writes.  Measured a little slower than
// two launches, so pn_sim_bodies_step enqueues it only when asked to.
template <bool ONE>
__global__ void __launch_bounds__(PN_BODY_THREADS) k_body_reaction(int n_k, int n_IP, pn_bodies_state* bs, pn_contact_state* cs, double dt, double dx3,
                                                                   const double* __restrict__ dof, const double* __restrict__ dof_vel,
                                                                   const int* __restrict__ topo, const double* __restrict__ rho,
                                                                   const double* __restrict__ Nx, double* part, unsigned* counter) {
    __shared__ double s_part[PN_BODY_WAVES][PN_BODY_PART];
    __shared__ double s_step[ONE ? PN_BODY_STEP_LDS : 1];   // the last workgroup's pn_body_step
    const int t = threadIdx.x, p = blockIdx.x * PN_BODY_THREADS + t;
    const int n = min(cs->n, PN_CONTACT_SLOTS);
    const bool on = bs->active != 0 && cs->active != 0;   // uniform over the launch
    double x[3], v[3];
    const bool have = on && p < n_IP && pn_ip_state(p, n_k, dof, dof_vel, topo, Nx, x, v);
    const double m = have ? rho[p] * dx3 : 0.0;
    const double kappa = cs->kappa, beta = cs->beta, mu = cs->mu, h = cs->h, dt2 = dt * dt;
    for (int b = 0; b < PN_BODIES_SLOTS; b++) {
        double f[4] = {0.0, 0.0, 0.0, 0.0};
        if (on && b < n && pn_body_dynamic(bs, cs, b)) {  // uniform over the launch: every lane takes part in the shuffles
            if (have) {
                double a[3] = {0.0, 0.0, 0.0}, delta = 0.0;
                if (pn_contact_collider_term(cs->c + b, kappa, beta, mu, h, dt, dt2, x, v, a, &delta)) {
                    f[0] = m * a[0]; f[1] = m * a[1]; f[2] = m * a[2]; f[3] = delta;
                }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                f[0] += __shfl_down(f[0], off); f[1] += __shfl_down(f[1], off); f[2] += __shfl_down(f[2], off);
                f[3] = fmax(f[3], __shfl_down(f[3], off));
            }
        }
        if ((t & 63) == 0) {
#pragma unroll
            for (int i = 0; i < 4; i++) s_part[t >> 6][b * 4 + i] = f[i];
        }
    }
    __syncthreads();
    if (t < PN_BODY_PART) {
        double s = s_part[0][t];
#pragma unroll
        for (int w = 1; w < PN_BODY_WAVES; w++) s = (t & 3) == 3 ? fmax(s, s_part[w][t]) : s + s_part[w][t];
        part[(size_t)blockIdx.x * PN_BODY_PART + t] = s;
    }
    if (ONE) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (t == 0) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const bool last = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
            if (last) {
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            s_part[0][0] = last ? 1.0 : 0.0;   // the one LDS array carries the verdict to the workgroup
        }
        __syncthreads();
        if (s_part[0][0] != 0.0) pn_body_step(t, (int)gridDim.x, bs, cs, dt, part, s_step);   // uniform over the workgroup
    }
}

// second launch of the two-launch form: one workgroup
__global__ void __launch_bounds__(PN_BODY_THREADS) k_body_step(int n_wg, pn_bodies_state* bs, pn_contact_state* cs, double dt, const double* part) {
    __shared__ double s_step[PN_BODY_STEP_LDS];
    pn_body_step(threadIdx.x, n_wg, bs, cs, dt, part, s_step);
}

extern "C" uint64_t pn_sim_bodies_bytes(void) { return sizeof(pn_bodies_state); }

extern "C" uint64_t pn_sim_bodies_work_bytes(int n_IP) {
    if (n_IP <= 0 || n_IP > (1 << 27)) return 0;
    return ((uint64_t)pn_div_up(n_IP, PN_BODY_THREADS) * PN_BODY_PART + 1) * sizeof(double);   // + the one-launch form's arrival counter
}

extern "C" int pn_sim_bodies_step(int n_k, int n_IP, void* state, void* contact_state, void* work, double dt, double dx, const double* dof,
                                  const double* dof_vel, const int* topo, const double* rho, const double* Nx, int one_launch, void* stream) {
    PN_REQUIRE(n_k > 0 && n_IP > 0 && n_IP <= (1 << 27) && state && contact_state && work && dof && dof_vel && topo && rho && Nx);
    PN_REQUIRE(isfinite(dt) && dt > 0.0 && isfinite(dx) && dx > 0.0 && (one_launch == 0 || one_launch == 1));
    const int n_wg = (int)pn_div_up(n_IP, PN_BODY_THREADS);
    hipStream_t s = (hipStream_t)stream;
    pn_bodies_state* bs = (pn_bodies_state*)state;
    pn_contact_state* cs = (pn_contact_state*)contact_state;
    double* part = (double*)work;
    unsigned* counter = (unsigned*)(part + (size_t)n_wg * PN_BODY_PART);
    const double dx3 = pow(dx, 3.0);
    if (one_launch) {
        k_body_reaction<true><<<n_wg, PN_BODY_THREADS, 0, s>>>(n_k, n_IP, bs, cs, dt, dx3, dof, dof_vel, topo, rho, Nx, part, counter);
    } else {  // two launches, the measured faster form
        k_body_reaction<false><<<n_wg, PN_BODY_THREADS, 0, s>>>(n_k, n_IP, bs, cs, dt, dx3, dof, dof_vel, topo, rho, Nx, part, counter);
        PN_LAUNCH_CHECK();
        k_body_step<<<1, PN_BODY_THREADS, 0, s>>>(n_wg, bs, cs, dt, part);
    }
    PN_LAUNCH_CHECK();
    return PN_OK;
}

// ------------------------------------------------------------------------------------------------ host-side updates
struct PnBodiesParams {
    int active, set;
    double g[3];
};

__global__ void k_bodies_params(pn_bodies_state* __restrict__ st, PnBodiesParams s) {
    if (s.active >= 0) st->active = s.active;
    if (s.set) {
        for (int i = 0; i < 3; i++) st->g[i] = s.g[i];
    }
}

extern "C" int pn_sim_bodies_set_params(void* state, int active, const double* gravity3_host, void* stream) {
    PN_REQUIRE(state && active >= -1 && active <= 1);
    PnBodiesParams s;
    s.active = active; s.set = gravity3_host != nullptr;
    for (int i = 0; i < 3; i++) {
        s.g[i] = gravity3_host ? gravity3_host[i] : 0.0;
        PN_REQUIRE(isfinite(s.g[i]));
    }
    k_bodies_params<<<1, 1, 0, (hipStream_t)stream>>>((pn_bodies_state*)state, s);
    PN_LAUNCH_CHECK();
    return PN_OK;
}

__global__ void k_bodies_body(pn_bodies_state* __restrict__ st, int slot, int dynamic, double M, double c) {
    pn_body* b = st->b + slot;
    const bool fresh = !dynamic || b->dynamic == 0;
    b->dynamic = dynamic; b->reserved = 0;
    b->M = dynamic ? M : 0.0; b->c = dynamic ? c : 0.0;
    if (fresh) {
        b->F[0] = b->F[1] = b->F[2] = 0.0;
        b->s = dynamic ? 1.0 : 0.0; b->delta_max = 0.0; b->clamped = 0;
    }
}

extern "C" int pn_sim_bodies_set_body(void* state, int slot, int dynamic, double mass, double damping, void* stream) {
    PN_REQUIRE(state && slot >= 0 && slot < PN_BODIES_SLOTS && (dynamic == 0 || dynamic == 1));
    if (dynamic) PN_REQUIRE(isfinite(mass) && mass > 0.0 && isfinite(damping) && damping >= 0.0);
    k_bodies_body<<<1, 1, 0, (hipStream_t)stream>>>((pn_bodies_state*)state, slot, dynamic, mass, damping);
    PN_LAUNCH_CHECK();
    return PN_OK;
}

struct PnBodyMotion {
    int slot, mask;
    double pv[6];
};

__global__ void k_bodies_motion(pn_contact_state* __restrict__ cs, PnBodyMotion s) {
    pn_contact_collider* c = cs->c + s.slot;
    for (int i = 0; i < 3; i++) {
        if (s.mask & 1) c->p[i] = s.pv[i];
        if (s.mask & 2) c->v[i] = s.pv[3 + i];
    }
}

extern "C" int pn_sim_bodies_set_motion(void* contact_state, int slot, int mask, const double* pv6_host, void* stream) {
    PN_REQUIRE(contact_state && pv6_host && slot >= 0 && slot < PN_BODIES_SLOTS && mask >= 1 && mask <= 3);
    PnBodyMotion s;
    s.slot = slot; s.mask = mask;
    for (int i = 0; i < 6; i++) {
        s.pv[i] = pv6_host[i];
        PN_REQUIRE(isfinite(s.pv[i]));
    }
    k_bodies_motion<<<1, 1, 0, (hipStream_t)stream>>>((pn_contact_state*)contact_state, s);
    PN_LAUNCH_CHECK();
    return PN_OK;
}

__global__ void k_bodies_clock(pn_bodies_state* __restrict__ st, int64_t k) { st->k = k; }

extern "C" int pn_sim_bodies_clock(void* state, int64_t k, void* stream) {
    PN_REQUIRE(state && k >= 0);
    k_bodies_clock<<<1, 1, 0, (hipStream_t)stream>>>((pn_bodies_state*)state, k);
    PN_LAUNCH_CHECK();
    return PN_OK;
}
