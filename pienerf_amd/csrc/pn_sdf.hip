// Mesh colliders: signed-distance grids (include/pienerf_hip.h: pn_sdf_build, pn_sdf_state, pn_sim_contact_sdf_rhs have the laws).
//
// Two device paths.  k_sdf_build fills a grid from a triangle mesh: one thread per node, every triangle visited by every node — exact distances by
// the closest point of each triangle, signs by the generalised winding number, so a marching-cubes mesh needs no adjacency and either orientation
// works.  k_sdf_points is contact's law against the placed grids: a thread per integration point samples the trilinear interpolant and its gradient
// and adds contact's own response (pn_contact_law.h) to the acceleration the analytic colliders left in `accel`, between pn_sim_contact_rhs's two
// launches (pn_contact.hip: pn_sim_contact_sdf_rhs).  The state is device memory, so a captured substep follows a collider moved by the host.
#include <math.h>

#include "pn_common.h"
#include "pn_contact_law.h"
#include "pn_sdf.h"
#include "pn_sim_rhs.h"

static_assert(sizeof(pn_sdf_slot) == 80, "pn_sdf_slot: 80 bytes (pienerf_amd/simulator/contact.py: SDF_SLOT_DTYPE)");
static_assert(sizeof(pn_sdf_state) == 328, "pn_sdf_state: 328 bytes (pienerf_amd/simulator/contact.py: SDF_STATE_DTYPE)");
static_assert(PN_SDF_SLOTS == 4, "pn_sdf_state: 4 slots");

#define PN_SDF_MAX_AXIS 512
#define PN_SDF_MAX_NODES (1 << 27)

static bool pn_sdf_res_ok(int nx, int ny, int nz) {
    return nx >= 2 && ny >= 2 && nz >= 2 && nx <= PN_SDF_MAX_AXIS && ny <= PN_SDF_MAX_AXIS && nz <= PN_SDF_MAX_AXIS &&
           (uint64_t)nx * (uint64_t)ny * (uint64_t)nz <= (uint64_t)PN_SDF_MAX_NODES;
}

// ------------------------------------------------------------------------------------------------ the builder
#define PN_SDF_BUILD_THREADS 256   // a brick of 8 x 8 x 4 nodes
#define PN_SDF_TILE 128            // triangles per LDS tile: 4 608 bytes

// The squared distance from the origin to the triangle with corners a, b, c, by the regions of its closest point.
__device__ __forceinline__ float pn_sdf_tri_dist2(const float a[3], const float b[3], const float c[3]) {
    const float ab0 = b[0] - a[0], ab1 = b[1] - a[1], ab2 = b[2] - a[2];
    const float ac0 = c[0] - a[0], ac1 = c[1] - a[1], ac2 = c[2] - a[2];
    const float d1 = -(ab0 * a[0] + ab1 * a[1] + ab2 * a[2]), d2 = -(ac0 * a[0] + ac1 * a[1] + ac2 * a[2]);
    float p0, p1, p2;
    if (d1 <= 0.0f && d2 <= 0.0f) {  // vertex a
        p0 = a[0]; p1 = a[1]; p2 = a[2];
        return p0 * p0 + p1 * p1 + p2 * p2;
    }
    const float d3 = -(ab0 * b[0] + ab1 * b[1] + ab2 * b[2]), d4 = -(ac0 * b[0] + ac1 * b[1] + ac2 * b[2]);
    if (d3 >= 0.0f && d4 <= d3) {  // vertex b
        p0 = b[0]; p1 = b[1]; p2 = b[2];
        return p0 * p0 + p1 * p1 + p2 * p2;
    }
    const float vc = d1 * d4 - d3 * d2;
    if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) {  // edge ab
        const float v = d1 / (d1 - d3);
        p0 = a[0] + v * ab0; p1 = a[1] + v * ab1; p2 = a[2] + v * ab2;
        return p0 * p0 + p1 * p1 + p2 * p2;
    }
    const float d5 = -(ab0 * c[0] + ab1 * c[1] + ab2 * c[2]), d6 = -(ac0 * c[0] + ac1 * c[1] + ac2 * c[2]);
    if (d6 >= 0.0f && d5 <= d6) {  // vertex c
        p0 = c[0]; p1 = c[1]; p2 = c[2];
        return p0 * p0 + p1 * p1 + p2 * p2;
    }
    const float vb = d5 * d2 - d1 * d6;
    if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) {  // edge ac
        const float w = d2 / (d2 - d6);
        p0 = a[0] + w * ac0; p1 = a[1] + w * ac1; p2 = a[2] + w * ac2;
        return p0 * p0 + p1 * p1 + p2 * p2;
    }
    const float va = d3 * d6 - d5 * d4;
    if (va <= 0.0f && (d4 - d3) >= 0.0f && (d5 - d6) >= 0.0f) {  // edge bc
        const float w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
        p0 = b[0] + w * (c[0] - b[0]); p1 = b[1] + w * (c[1] - b[1]); p2 = b[2] + w * (c[2] - b[2]);
        return p0 * p0 + p1 * p1 + p2 * p2;
    }
    const float denom = 1.0f / (va + vb + vc);  // the face
    const float v = vb * denom, w = vc * denom;
    p0 = a[0] + ab0 * v + ac0 * w; p1 = a[1] + ab1 * v + ac1 * w; p2 = a[2] + ab2 * v + ac2 * w;
    return p0 * p0 + p1 * p1 + p2 * p2;
}

// 2 atan2(a.(b x c), |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|): the solid angle of the triangle seen from the origin
__device__ __forceinline__ float pn_sdf_tri_angle(const float a[3], const float b[3], const float c[3]) {
    const float la = sqrtf(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    const float lb = sqrtf(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
    const float lc = sqrtf(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
    const float x0 = b[1] * c[2] - b[2] * c[1], x1 = b[2] * c[0] - b[0] * c[2], x2 = b[0] * c[1] - b[1] * c[0];
    const float det = a[0] * x0 + a[1] * x1 + a[2] * x2;
    const float ab = a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
    const float bc = b[0] * c[0] + b[1] * c[1] + b[2] * c[2];
    const float ca = c[0] * a[0] + c[1] * a[1] + c[2] * a[2];
    return 2.0f * atan2f(det, la * lb * lc + ab * lc + bc * la + ca * lb);
}

struct PnSdfBox {
    double lo[3], s;
    int nx, ny, nz;
};

__global__ void __launch_bounds__(PN_SDF_BUILD_THREADS) k_sdf_build(const float* __restrict__ tri9, int n_tris, PnSdfBox g, float* __restrict__ grid,
                                                                    double* __restrict__ winding_out) {
    __shared__ float s_tri[PN_SDF_TILE * 9];
    const int t = threadIdx.x;
    const int i = blockIdx.x * 8 + (t & 7), j = blockIdx.y * 8 + ((t >> 3) & 7), k = blockIdx.z * 4 + (t >> 6);
    const bool valid = i < g.nx && j < g.ny && k < g.nz;  // a ragged last brick: its spare threads stage triangles and write nothing
    const float q0 = (float)(g.lo[0] + g.s * (double)i), q1 = (float)(g.lo[1] + g.s * (double)j), q2 = (float)(g.lo[2] + g.s * (double)k);
    float best = INFINITY;
    double wsum = 0.0;
    for (int base = 0; base < n_tris; base += PN_SDF_TILE) {
        const int cnt = min(PN_SDF_TILE, n_tris - base);
        __syncthreads();  // the tile before this one has been read by every wave
        for (int e = t; e < cnt * 9; e += PN_SDF_BUILD_THREADS) s_tri[e] = tri9[(size_t)base * 9 + e];
        __syncthreads();
        if (valid) {
            for (int m = 0; m < cnt; m++) {  // every lane reads the same address: an LDS broadcast
                const float* T = s_tri + m * 9;
                const float a[3] = {T[0] - q0, T[1] - q1, T[2] - q2};
                const float b[3] = {T[3] - q0, T[4] - q1, T[5] - q2};
                const float c[3] = {T[6] - q0, T[7] - q1, T[8] - q2};
                best = fminf(best, pn_sdf_tri_dist2(a, b, c));  // fminf drops a NaN from a sliver's face region
                wsum += (double)pn_sdf_tri_angle(a, b, c);
            }
        }
    }
    if (!valid) return;
    const double w = wsum / (4.0 * 3.14159265358979323846);
    const float dist = sqrtf(best);
    const size_t node = ((size_t)k * g.ny + j) * g.nx + i;
    grid[node] = fabs(w) >= 0.5 ? -dist : dist;
    if (winding_out) winding_out[node] = w;
}

extern "C" int pn_sdf_build(const float* tri9, int n_tris, int nx, int ny, int nz, const double* lo3_host, double spacing, float* grid,
                            double* winding_out, void* stream) {
    PN_REQUIRE(tri9 && grid && lo3_host && n_tris >= 1 && n_tris <= (1 << 24));
    PN_REQUIRE(pn_sdf_res_ok(nx, ny, nz));
    PN_REQUIRE((uint64_t)nx * (uint64_t)ny * (uint64_t)nz * (uint64_t)n_tris <= PN_SDF_MAX_PAIRS);  // one launch, nodes x triangles: keep it to seconds
    PN_REQUIRE(isfinite(spacing) && spacing > 0.0 && isfinite(lo3_host[0]) && isfinite(lo3_host[1]) && isfinite(lo3_host[2]));
    PnSdfBox g;
    for (int a = 0; a < 3; a++) g.lo[a] = lo3_host[a];
    g.s = spacing; g.nx = nx; g.ny = ny; g.nz = nz;
    const dim3 bricks(pn_div_up(nx, 8), pn_div_up(ny, 8), pn_div_up(nz, 4));
    k_sdf_build<<<bricks, PN_SDF_BUILD_THREADS, 0, (hipStream_t)stream>>>(tri9, n_tris, g, grid, winding_out);
    PN_LAUNCH_CHECK();
    return PN_OK;
}

// ------------------------------------------------------------------------------------------------ contact against the placed grids
__device__ __forceinline__ double pn_sdf_lerp(double a, double b, double f) { return a + f * (b - a); }

// One slot's part at a point x with velocity v: the trilinear distance and the unit gradient, then contact's response.  A point outside the grid's
// box, or not finite, gets nothing.  Every read lies inside the grid: 0 <= i0 <= n - 2 on every axis.
__device__ __forceinline__ bool pn_sdf_slot_term(const pn_sdf_slot* __restrict__ c, double kappa, double beta, double mu, double h, double dt, double dt2,
                                                 const double x[3], const double v[3], double a[3]) {
    const float* __restrict__ G = c->grid;
    const int nx = c->nx, ny = c->ny, nz = c->nz;
    if (!G || nx < 2 || ny < 2 || nz < 2) return false;
    const double s = c->s;
    const double u0 = (x[0] - c->lo[0]) / s, u1 = (x[1] - c->lo[1]) / s, u2 = (x[2] - c->lo[2]) / s;
    if (!(u0 >= 0.0 && u0 < (double)(nx - 1) && u1 >= 0.0 && u1 < (double)(ny - 1) && u2 >= 0.0 && u2 < (double)(nz - 1))) return false;  // NaN fails too
    const int i0 = (int)floor(u0), j0 = (int)floor(u1), k0 = (int)floor(u2);
    const double f0 = u0 - (double)i0, f1 = u1 - (double)j0, f2 = u2 - (double)k0;
    const float* R = G + ((size_t)k0 * ny + j0) * nx + i0;
    const size_t sy = (size_t)nx, sz = (size_t)nx * ny;
    const double v000 = R[0], v100 = R[1], v010 = R[sy], v110 = R[sy + 1];
    const double v001 = R[sz], v101 = R[sz + 1], v011 = R[sz + sy], v111 = R[sz + sy + 1];
    const double c00 = pn_sdf_lerp(v000, v100, f0), c10 = pn_sdf_lerp(v010, v110, f0), c01 = pn_sdf_lerp(v001, v101, f0), c11 = pn_sdf_lerp(v011, v111, f0);
    const double c0 = pn_sdf_lerp(c00, c10, f1), c1 = pn_sdf_lerp(c01, c11, f1);
    const double d = pn_sdf_lerp(c0, c1, f2);
    const double g0 = pn_sdf_lerp(pn_sdf_lerp(v100 - v000, v110 - v010, f1), pn_sdf_lerp(v101 - v001, v111 - v011, f1), f2);
    const double g1 = pn_sdf_lerp(c10 - c00, c11 - c01, f2);
    const double g2 = c1 - c0;
    const double L = sqrt(g0 * g0 + g1 * g1 + g2 * g2);
    double nh[3] = {0.0, 1.0, 0.0};
    if (L > 0.0) { nh[0] = g0 / L; nh[1] = g1 / L; nh[2] = g2 / L; }
    double delta;
    return pn_contact_response(nh, d, c->v, kappa, beta, mu, h, dt, dt2, v, a, &delta);
}

#define PN_SDF_POINT_THREADS 64   // as k_contact_points: one wave per workgroup, spread over the CUs
__global__ void __launch_bounds__(PN_SDF_POINT_THREADS) k_sdf_points(int n_k, int n_IP, const pn_contact_state* __restrict__ st,
                                                                     const pn_sdf_state* __restrict__ sdf, double dt, const double* __restrict__ dof,
                                                                     const double* __restrict__ dof_vel, const int* __restrict__ topo,
                                                                     const double* __restrict__ Nx, double* __restrict__ accel) {
    const int p = blockIdx.x * PN_SDF_POINT_THREADS + threadIdx.x;
    if (p >= n_IP) return;
    const int n = min(sdf->n, PN_SDF_SLOTS);
    if (st->active == 0 || n <= 0) return;
    double x[3], v[3];
    if (!pn_ip_state(p, n_k, dof, dof_vel, topo, Nx, x, v)) return;
    double a[3] = {accel[(size_t)p * 3], accel[(size_t)p * 3 + 1], accel[(size_t)p * 3 + 2]};  // what the analytic colliders left: the sum goes on
    const double kappa = st->kappa, beta = st->beta, mu = st->mu, h = st->h, dt2 = dt * dt;
    bool hit = false;
    for (int c = 0; c < n; c++)
        if (pn_sdf_slot_term(sdf->c + c, kappa, beta, mu, h, dt, dt2, x, v, a)) hit = true;
    if (!hit) return;  // the point keeps its bits
    accel[(size_t)p * 3] = a[0]; accel[(size_t)p * 3 + 1] = a[1]; accel[(size_t)p * 3 + 2] = a[2];
}

int pn_sdf_points_launch(int n_k, int n_IP, const pn_contact_state* st, const pn_sdf_state* sdf, double dt, const double* dof, const double* dof_vel,
                         const int* topo, const double* Nx, double* accel, hipStream_t stream) {
    k_sdf_points<<<pn_div_up(n_IP, PN_SDF_POINT_THREADS), PN_SDF_POINT_THREADS, 0, stream>>>(n_k, n_IP, st, sdf, dt, dof, dof_vel, topo, Nx, accel);
    PN_LAUNCH_CHECK();
    return PN_OK;
}

// ------------------------------------------------------------------------------------------------ host-side updates
extern "C" uint64_t pn_sim_sdf_bytes(void) { return sizeof(pn_sdf_state); }

struct PnSdfSet {
    int index;
    pn_sdf_slot slot;
};

// writes the slot, then n = 1 + the highest slot in use
__global__ void k_sdf_set(pn_sdf_state* __restrict__ st, PnSdfSet s) {
    st->c[s.index] = s.slot;
    int n = 0;
    for (int i = 0; i < PN_SDF_SLOTS; i++)
        if (st->c[i].grid != nullptr) n = i + 1;
    st->n = n;
    st->reserved = 0;
}

extern "C" int pn_sim_sdf_set_collider(void* state, int index, const float* grid, int nx, int ny, int nz, const double* geom7_host, void* stream) {
    PN_REQUIRE(state && index >= 0 && index < PN_SDF_SLOTS);
    PnSdfSet s;
    memset(&s, 0, sizeof(s));
    s.index = index;
    if (grid) {
        PN_REQUIRE(geom7_host && pn_sdf_res_ok(nx, ny, nz));
        for (int i = 0; i < 7; i++) PN_REQUIRE(isfinite(geom7_host[i]));
        PN_REQUIRE(geom7_host[3] > 0.0);
        s.slot.grid = grid; s.slot.nx = nx; s.slot.ny = ny; s.slot.nz = nz;
        for (int i = 0; i < 3; i++) { s.slot.lo[i] = geom7_host[i]; s.slot.v[i] = geom7_host[4 + i]; }
        s.slot.s = geom7_host[3];
    }
    k_sdf_set<<<1, 1, 0, (hipStream_t)stream>>>((pn_sdf_state*)state, s);
    PN_LAUNCH_CHECK();
    return PN_OK;
}
