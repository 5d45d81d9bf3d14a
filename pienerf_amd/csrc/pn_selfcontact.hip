// Self-contact: the body collides with itself and with its own pieces (include/pienerf_hip.h: pn_selfcontact_state).
//
// Contact against analytic colliders (pn_contact.hip) gave the body an outside; this stage gives it an inside, with the same construction: an explicit
// penalty on the right-hand side, evaluated at the integration points from the dof / dof_vel the substep starts from, the matrix, Ainv and the
// substep's kernels untouched.  What is new is the neighbour search over the DEFORMED points: every call rebuilds a hashed grid of cell size h on the
// device (count, scan, fill, sort), and two gather passes over a point's 27 cells give the point sums S_i and then the accelerations a_i.  Every
// floating-point sum runs in an order that is a function of the points' ids and cells alone: integer atomics place the points, a sort by id undoes
// their order, and no floating-point value goes through an atomic.  A bucket with more than PN_SELF_BUCKET_CAP points switches the call off
// (rhs_out = rhs_in) and counts it in the state, so the cost of a call is bounded however far a run has blown up.
#include <math.h>

#include "pn_common.h"
#include "pn_sim_rhs.h"

static_assert(sizeof(pn_selfcontact_state) == 56, "pn_selfcontact_state: 56 bytes (pienerf_amd/simulator/selfcontact.py: SELF_STATE_DTYPE)");
static_assert(PN_SELF_BUCKET_CAP == 64, "pn_selfcontact_state: 64 points per bucket");

#define PN_SELF_THREADS 256   // four waves per GMLS kernel in the per-kernel sum; fixed: the order of the sum must not depend on the device
#define PN_SELF_POINT_THREADS 64    // as k_contact_points: workgroups of one wave, spread over the CUs
#define PN_SELF_SCAN_THREADS 1024   // the scan is one workgroup; T is a power of two >= 1024, so every thread owns T / 1024 buckets in a row
#define PN_SELF_CELL_MAX (1 << 30)

// T: the smallest power of two >= max(1024, 2 n_IP)
static inline uint32_t pn_self_buckets(int n_IP) {
    uint32_t T = 1024;
    while (T < 2u * (uint32_t)n_IP) T <<= 1;
    return T;
}

// The work area, carved in this order: doubles first, then the integer tables.
struct PnSelfWork {
    double* xv;      // [n, 6]: x_i, v_i
    double* S;       // [n]
    double* a;       // [n, 3]: used when the caller passes no accel_out
    int* cell;       // [n, 4]: cx, cy, cz, bucket (-1: the point takes no part)
    int* tmp;        // [n]: the buckets' members as the atomics placed them
    int* items;      // [n]: ... and in ascending point id
    int* count;      // [T]: points per bucket
    int* start;      // [T + 1]: exclusive scan of count
    int* flag;       // [2]: flag[0] != 0: the call adds nothing (a bucket over the cap)
};

static inline uint64_t pn_self_carve(PnSelfWork* w, void* base, int n_IP) {
    const uint64_t n = (uint64_t)n_IP, T = pn_self_buckets(n_IP);
    char* p = (char*)base;
    uint64_t o = 0;
    w->xv = (double*)(p + o); o += n * 6 * 8;
    w->S = (double*)(p + o); o += n * 8;
    w->a = (double*)(p + o); o += n * 3 * 8;
    w->cell = (int*)(p + o); o += n * 4 * 4;
    w->tmp = (int*)(p + o); o += n * 4;
    w->items = (int*)(p + o); o += n * 4;
    w->count = (int*)(p + o); o += T * 4;
    w->start = (int*)(p + o); o += (T + 1) * 4;
    w->flag = (int*)(p + o); o += 2 * 4;
    return (o + 7) & ~(uint64_t)7;
}

__device__ __forceinline__ uint32_t pn_self_bucket(int cx, int cy, int cz, uint32_t mask) {
    return ((uint32_t)cx * 73856093u ^ (uint32_t)cy * 19349663u ^ (uint32_t)cz * 83492791u) & mask;
}

// floor(x / h) clamped to [-2^30, 2^30]; x is finite, h > 0
__device__ __forceinline__ int pn_self_cell(double x, double h) {
    const double c = floor(x / h);
    return (int)fmin(fmax(c, -(double)PN_SELF_CELL_MAX), (double)PN_SELF_CELL_MAX);
}

// |X_i - X_j| >= rho_x, each operation rounded once in this order: a decision, so it must not depend on what the compiler contracts
__device__ __forceinline__ bool pn_self_eligible(const double* __restrict__ Xi, const double* __restrict__ Xj, double rho_x) {
#pragma clang fp contract(off)
    const double d0 = Xi[0] - Xj[0], d1 = Xi[1] - Xj[1], d2 = Xi[2] - Xj[2];
    const double q0 = d0 * d0, q1 = d1 * d1, q2 = d2 * d2;
    const double q = (q0 + q1) + q2;
    return sqrt(q) >= rho_x;
}

// ------------------------------------------------------------------------------------------------ 1: points and cells; the counts zeroed
// One thread per integration point (and per bucket: the grid covers max(n_IP, T)): x_i and v_i (pn_ip_state), the point's cell and
// bucket; a point with a non-finite x or v gets bucket -1 and takes no part.
__global__ void __launch_bounds__(PN_SELF_POINT_THREADS) k_self_points(int n_k, int n_IP, uint32_t T, const pn_selfcontact_state* __restrict__ st,
                                                                       const double* __restrict__ dof, const double* __restrict__ dof_vel,
                                                                       const int* __restrict__ topo, const double* __restrict__ Nx, PnSelfWork w) {
    if (st->active == 0) return;
    const uint32_t p = blockIdx.x * PN_SELF_POINT_THREADS + threadIdx.x;
    if (p < T) w.count[p] = 0;
    if (p >= (uint32_t)n_IP) return;
    double x[3], v[3];
    const bool ok = pn_ip_state((int)p, n_k, dof, dof_vel, topo, Nx, x, v) && isfinite(x[0]) && isfinite(x[1]) && isfinite(x[2]) && isfinite(v[0]) &&
                    isfinite(v[1]) && isfinite(v[2]);
    int c[4] = {0, 0, 0, -1};
    if (ok) {
        const double h = st->h;
        c[0] = pn_self_cell(x[0], h); c[1] = pn_self_cell(x[1], h); c[2] = pn_self_cell(x[2], h);
        c[3] = (int)pn_self_bucket(c[0], c[1], c[2], T - 1);
    }
#pragma unroll
    for (int i = 0; i < 3; i++) {
        w.xv[(size_t)p * 6 + i] = x[i];
        w.xv[(size_t)p * 6 + 3 + i] = v[i];
    }
#pragma unroll
    for (int i = 0; i < 4; i++) w.cell[(size_t)p * 4 + i] = c[i];
}

// ------------------------------------------------------------------------------------------------ 2: count
__global__ void __launch_bounds__(PN_SELF_POINT_THREADS) k_self_count(int n_IP, const pn_selfcontact_state* __restrict__ st, PnSelfWork w) {
    if (st->active == 0) return;
    const int p = blockIdx.x * PN_SELF_POINT_THREADS + threadIdx.x;
    if (p >= n_IP) return;
    const int b = w.cell[(size_t)p * 4 + 3];
    if (b >= 0) atomicAdd(&w.count[b], 1);   // integers: the sum does not depend on the order
}

// ------------------------------------------------------------------------------------------------ 3: scan, and the overflow decision
// One workgroup.  Thread t owns the buckets t per .. (t + 1) per - 1: it adds their counts, the 1024 partial sums are scanned in LDS, and it writes
// start[] for its buckets; count[] is left at zero to serve the fill as a cursor.  A bucket over the cap sets flag[0] and counts the call in the state.
__global__ void __launch_bounds__(PN_SELF_SCAN_THREADS) k_self_scan(uint32_t T, pn_selfcontact_state* __restrict__ st, PnSelfWork w) {
    __shared__ int s_sum[PN_SELF_SCAN_THREADS];
    const int t = threadIdx.x;
    if (st->active == 0) {  // uniform
        if (t == 0) w.flag[0] = 0;
        return;
    }
    const uint32_t per = T / PN_SELF_SCAN_THREADS, b0 = (uint32_t)t * per;
    int sum = 0, over = 0;
    for (uint32_t b = b0; b < b0 + per; b++) {
        const int c = w.count[b];
        over |= c > PN_SELF_BUCKET_CAP;
        sum += c;
    }
    s_sum[t] = sum;
    over = __syncthreads_or(over);
    for (int off = 1; off < PN_SELF_SCAN_THREADS; off <<= 1) {  // inclusive scan of the partial sums
        const int add = t >= off ? s_sum[t - off] : 0;
        __syncthreads();
        s_sum[t] += add;
        __syncthreads();
    }
    int run = s_sum[t] - sum;
    for (uint32_t b = b0; b < b0 + per; b++) {
        const int c = w.count[b];
        w.start[b] = run;
        run += c;
        w.count[b] = 0;
    }
    if (t == PN_SELF_SCAN_THREADS - 1) w.start[T] = run;
    if (t == 0) {
        w.flag[0] = over ? 1 : 0;
        if (over) st->overflowed += 1;
    }
}

// ------------------------------------------------------------------------------------------------ 4: fill
__global__ void __launch_bounds__(PN_SELF_POINT_THREADS) k_self_fill(int n_IP, const pn_selfcontact_state* __restrict__ st, PnSelfWork w) {
    if (st->active == 0 || w.flag[0] != 0) return;
    const int p = blockIdx.x * PN_SELF_POINT_THREADS + threadIdx.x;
    if (p >= n_IP) return;
    const int b = w.cell[(size_t)p * 4 + 3];
    if (b < 0) return;
    const int at = w.start[b] + atomicAdd(&w.count[b], 1);
    if ((unsigned)at < (unsigned)n_IP) w.tmp[at] = p;   // always: the counts sum to at most n_IP
}

// ------------------------------------------------------------------------------------------------ 5: every bucket in ascending point id
// One thread per point: its rank among its bucket's members (at most the cap of them) is its place.  After this the table no longer depends on the
// order in which the atomics of the fill were served.
__global__ void __launch_bounds__(PN_SELF_POINT_THREADS) k_self_sort(int n_IP, const pn_selfcontact_state* __restrict__ st, PnSelfWork w) {
    if (st->active == 0 || w.flag[0] != 0) return;
    const int p = blockIdx.x * PN_SELF_POINT_THREADS + threadIdx.x;
    if (p >= n_IP) return;
    const int b = w.cell[(size_t)p * 4 + 3];
    if (b < 0) return;
    const int s = max(w.start[b], 0), e = min(w.start[b + 1], n_IP);
    int rank = 0;
    for (int k = s; k < e; k++) rank += w.tmp[k] < p;
    if (s + rank < e) w.items[s + rank] = p;
}

// ------------------------------------------------------------------------------------------------ the walk over a point's partners
// Calls f(j, delta, L, r) for every eligible partner j of point i with delta > 0, in the order of the header's text: the 27 cells c + (ox, oy, oz),
// oz outermost, each offset -1, 0, 1; inside a bucket ascending j; j is accepted only where its own cell equals the visited one.
template <typename F>
__device__ __forceinline__ void pn_self_walk(int i, int n_IP, uint32_t T, double h, double rho_x, const double* __restrict__ X_rest, const PnSelfWork& w, F f) {
    const int* ci = w.cell + (size_t)i * 4;
    const int c0 = ci[0], c1 = ci[1], c2 = ci[2];
    const double x0 = w.xv[(size_t)i * 6], x1 = w.xv[(size_t)i * 6 + 1], x2 = w.xv[(size_t)i * 6 + 2];
    const double far2 = h * h * (1.0 + 1e-9);
    for (int oz = -1; oz <= 1; oz++)
        for (int oy = -1; oy <= 1; oy++)
            for (int ox = -1; ox <= 1; ox++) {
                const int v0 = c0 + ox, v1 = c1 + oy, v2 = c2 + oz;
                const uint32_t b = pn_self_bucket(v0, v1, v2, T - 1);
                const int s = max(w.start[b], 0), e = min(w.start[b + 1], n_IP);
                for (int k = s; k < e; k++) {
                    const int j = w.items[k];
                    if (j == i || (unsigned)j >= (unsigned)n_IP) continue;
                    const int* cj = w.cell + (size_t)j * 4;
                    if (cj[0] != v0 || cj[1] != v1 || cj[2] != v2) continue;
                    double r[3] = {x0 - w.xv[(size_t)j * 6], x1 - w.xv[(size_t)j * 6 + 1], x2 - w.xv[(size_t)j * 6 + 2]};
                    const double q = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
                    if (!(q < far2)) continue;   // surely L >= h (the margin covers the square root's rounding): most candidates end here, before the rest positions are read
                    if (!pn_self_eligible(X_rest + (size_t)i * 3, X_rest + (size_t)j * 3, rho_x)) continue;
                    const double L = sqrt(q);
                    const double delta = h - L;
                    if (!(delta > 0.0)) continue;
                    f(j, delta, L, r);
                }
            }
}

// ------------------------------------------------------------------------------------------------ 6: S_i
__global__ void __launch_bounds__(PN_SELF_POINT_THREADS) k_self_sums(int n_IP, uint32_t T, const pn_selfcontact_state* __restrict__ st,
                                                                     const double* __restrict__ X_rest, PnSelfWork w) {
    if (st->active == 0 || w.flag[0] != 0) return;
    const int i = blockIdx.x * PN_SELF_POINT_THREADS + threadIdx.x;
    if (i >= n_IP) return;
    double S = 0.0;
    if (w.cell[(size_t)i * 4 + 3] >= 0) pn_self_walk(i, n_IP, T, st->h, st->rho_x, X_rest, w, [&](int, double delta, double, const double*) { S += delta; });
    w.S[i] = S;
}

// ------------------------------------------------------------------------------------------------ 7: a_i
// accel[i] = a_i; zeros for a point without a partner and for every point of an inactive or overflowed call.
__global__ void __launch_bounds__(PN_SELF_POINT_THREADS) k_self_accel(int n_IP, uint32_t T, const pn_selfcontact_state* __restrict__ st, double dt, double dx3,
                                                                      const double* __restrict__ X_rest, const double* __restrict__ rho, PnSelfWork w,
                                                                      double* __restrict__ accel) {
    const int i = blockIdx.x * PN_SELF_POINT_THREADS + threadIdx.x;
    if (i >= n_IP) return;
    double a[3] = {0.0, 0.0, 0.0};
    if (st->active != 0 && w.flag[0] == 0 && w.cell[(size_t)i * 4 + 3] >= 0 && w.S[i] > 0.0) {
        const double kappa = st->kappa, beta = st->beta, mu = st->mu, dt2 = dt * dt;
        const double Si = w.S[i], mi = rho[i] * dx3;
        const double vi0 = w.xv[(size_t)i * 6 + 3], vi1 = w.xv[(size_t)i * 6 + 4], vi2 = w.xv[(size_t)i * 6 + 5];
        pn_self_walk(i, n_IP, T, st->h, st->rho_x, X_rest, w, [&](int j, double delta, double L, const double* r) {
            double nh[3];
            if (L > 0.0) {
                nh[0] = r[0] / L; nh[1] = r[1] / L; nh[2] = r[2] / L;
            } else {
                nh[0] = 0.0; nh[1] = i < j ? 1.0 : -1.0; nh[2] = 0.0;
            }
            const double wij = delta / fmax(Si, w.S[j]);
            const double w0 = vi0 - w.xv[(size_t)j * 6 + 3], w1 = vi1 - w.xv[(size_t)j * 6 + 4], w2 = vi2 - w.xv[(size_t)j * 6 + 5];
            const double wn = w0 * nh[0] + w1 * nh[1] + w2 * nh[2];
            const double t0 = w0 - wn * nh[0], t1 = w1 - wn * nh[1], t2 = w2 - wn * nh[2];
            const double g = wij * (kappa * delta + beta * fmin(fmax(-wn, 0.0) * dt, delta)) / dt2;
            double f0 = g * nh[0], f1 = g * nh[1], f2 = g * nh[2];
            const double wt = sqrt(t0 * t0 + t1 * t1 + t2 * t2);
            if (wt > 0.0) {
                const double gt = fmin(mu * g, wij * wt / dt), s = gt / wt;
                f0 -= s * t0; f1 -= s * t1; f2 -= s * t2;
            }
            const double mj = rho[j] * dx3, share = mj / (mi + mj);
            a[0] += share * f0; a[1] += share * f1; a[2] += share * f2;
        });
    }
    accel[(size_t)i * 3] = a[0]; accel[(size_t)i * 3 + 1] = a[1]; accel[(size_t)i * 3 + 2] = a[2];
}

// ------------------------------------------------------------------------------------------------ 8: the right-hand side
// rhs_out = rhs_in + the self-contact term: pn_kernel_accel_term (pn_sim_rhs.h), one workgroup of four waves per GMLS kernel, a read from `accel`.
// Every kernel of an inactive or overflowed call copies rhs_in's bits.
__global__ void __launch_bounds__(PN_SELF_THREADS) k_self_rhs(int n_IP, const pn_selfcontact_state* __restrict__ st, const int* __restrict__ flag, double dx3,
                                                              const double* __restrict__ rho, const int* __restrict__ kernel_bg,
                                                              const int* __restrict__ kernel_cnt, const int* __restrict__ buffer,
                                                              const double* __restrict__ Nx_csr, const double* __restrict__ rhs_in,
                                                              double* __restrict__ rhs_out, const double* __restrict__ accel) {
    const bool on = st->active != 0 && flag[0] == 0;  // uniform over the launch
    pn_kernel_accel_term<PN_SELF_THREADS>(blockIdx.x, threadIdx.x, on, n_IP, dx3, rho, kernel_bg, kernel_cnt, buffer, Nx_csr, rhs_in, rhs_out,
                                          PnAccelRead{accel});
}

extern "C" uint64_t pn_sim_self_bytes(void) { return sizeof(pn_selfcontact_state); }

extern "C" uint64_t pn_sim_self_work_bytes(int n_IP) {
    if (n_IP <= 0 || n_IP > (1 << 27)) return 0;
    PnSelfWork w;
    return pn_self_carve(&w, nullptr, n_IP);
}

extern "C" int pn_sim_self_launches(void) { return 8; }

extern "C" int pn_sim_self_rhs(int n_k, int n_IP, void* state, void* work, double dt, double dx, const double* dof, const double* dof_vel,
                               const double* X_rest, const int* topo, const double* rho, const double* Nx, const int* kernel_bg, const int* kernel_cnt,
                               const int* buffer, const double* Nx_csr, const double* rhs_in, double* rhs_out, double* accel_out, void* stream) {
    PN_REQUIRE(n_k > 0 && n_IP > 0 && n_IP <= (1 << 27) && state && work && dof && dof_vel && X_rest && topo && rho && Nx && kernel_bg && kernel_cnt &&
               buffer && Nx_csr);
    PN_REQUIRE(rhs_in && rhs_out && rhs_in != rhs_out);
    PN_REQUIRE(isfinite(dt) && dt > 0.0 && isfinite(dx) && dx > 0.0);
    pn_selfcontact_state* st = (pn_selfcontact_state*)state;
    PnSelfWork w;
    pn_self_carve(&w, work, n_IP);
    double* accel = accel_out ? accel_out : w.a;
    const uint32_t T = pn_self_buckets(n_IP);
    const double dx3 = pow(dx, 3.0);
    hipStream_t s = (hipStream_t)stream;
    const uint32_t g_pts = pn_div_up(n_IP, PN_SELF_POINT_THREADS);
    k_self_points<<<pn_div_up(std::max<uint64_t>(n_IP, T), PN_SELF_POINT_THREADS), PN_SELF_POINT_THREADS, 0, s>>>(n_k, n_IP, T, st, dof, dof_vel, topo, Nx, w);
    PN_LAUNCH_CHECK();
    k_self_count<<<g_pts, PN_SELF_POINT_THREADS, 0, s>>>(n_IP, st, w);
    PN_LAUNCH_CHECK();
    k_self_scan<<<1, PN_SELF_SCAN_THREADS, 0, s>>>(T, st, w);
    PN_LAUNCH_CHECK();
    k_self_fill<<<g_pts, PN_SELF_POINT_THREADS, 0, s>>>(n_IP, st, w);
    PN_LAUNCH_CHECK();
    k_self_sort<<<g_pts, PN_SELF_POINT_THREADS, 0, s>>>(n_IP, st, w);
    PN_LAUNCH_CHECK();
    k_self_sums<<<g_pts, PN_SELF_POINT_THREADS, 0, s>>>(n_IP, T, st, X_rest, w);
    PN_LAUNCH_CHECK();
    k_self_accel<<<g_pts, PN_SELF_POINT_THREADS, 0, s>>>(n_IP, T, st, dt, dx3, X_rest, rho, w, accel);
    PN_LAUNCH_CHECK();
    k_self_rhs<<<n_k, PN_SELF_THREADS, 0, s>>>(n_IP, st, w.flag, dx3, rho, kernel_bg, kernel_cnt, buffer, Nx_csr, rhs_in, rhs_out, accel);
    PN_LAUNCH_CHECK();
    return PN_OK;
}

// ------------------------------------------------------------------------------------------------ host-side updates
struct PnSelfParams {
    int active, set;
    double p[5];
};

__global__ void k_self_params(pn_selfcontact_state* __restrict__ st, PnSelfParams s) {
    if (s.active >= 0) st->active = s.active;
    if (s.set) {
        st->kappa = s.p[0]; st->beta = s.p[1]; st->mu = s.p[2]; st->h = s.p[3]; st->rho_x = s.p[4];
    }
}

extern "C" int pn_sim_self_set_params(void* state, int active, const double* params5_host, void* stream) {
    PN_REQUIRE(state && active >= -1 && active <= 1);
    PnSelfParams s;
    s.active = active; s.set = params5_host != nullptr;
    for (int i = 0; i < 5; i++) {
        s.p[i] = params5_host ? params5_host[i] : 0.0;
        PN_REQUIRE(isfinite(s.p[i]));
    }
    if (params5_host) {  // the pair's relative response is at most (kappa + beta) delta w_ij: contact's stability argument
        PN_REQUIRE(s.p[0] > 0.0 && s.p[0] <= 1.0);
        PN_REQUIRE(s.p[1] >= 0.0 && s.p[1] <= 1.0);
        PN_REQUIRE(s.p[2] >= 0.0 && s.p[3] > 0.0 && s.p[4] >= s.p[3]);
    }
    k_self_params<<<1, 1, 0, (hipStream_t)stream>>>((pn_selfcontact_state*)state, s);
    PN_LAUNCH_CHECK();
    return PN_OK;
}
