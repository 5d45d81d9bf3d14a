// Simulator diagnostics (simulator/diagnostics.py: Simulator.diagnostics): what a state of the simulator holds, as one row of PN_DIAG_DOUBLES doubles —
// mass, centre of mass, linear and angular momentum, kinetic / gravitational / elastic energy, the extrema of the singular values, det F, strain and
// speed with the integration point that attains each, and the counts of non-finite and inverted points.  The law is written down once, in
// include/pienerf_hip.h (pn_sim_diagnostics) and DESIGN.md 4.18; the energies are the ones the solver's own matrix stands for (build_IP_global,
// simulator/cuda_utils.py:48-55 of the reference).  A readout: it reads dof / dof_vel and the tables and writes its own buffers only.
//
// Two launches, no atomics: the bits of the row are a function of the tables and the state alone.
//   k_diag_points   EIGHT LANES PER POINT, one per neighbour kernel, PN_DIAG_IPS points per workgroup.  A lane forms its kernel's share of F, G (the
//                   substep's ip_F_partial, on dof and on dof_vel) and of the 27 second derivatives H (pn_ip_row_acc, three at a time, so that only
//                   |H|^2 stays in registers beside the SVD), the shares are added over the lanes ^1, ^2, ^4 as the substep's forms add theirs, and
//                   the point's position and velocity are pn_ip_state's (pn_sim_rhs.h: the bits contact, the fields and self-contact see).  Every lane
//                   of a point then holds the same F, G, |H|^2 and runs the same converged cold-start Jacobi svd3 (pn_sim_svd.h) — never the McAdams
//                   approximation, whatever the solver runs: this is a measurement.  Lane 0 of each point enters the point's terms into a fixed
//                   shuffle tree over the wave (32, 16 ... 1, as pn_wave_sum30), lane 0 of each wave puts the wave's totals into LDS and the waves are
//                   added in ascending order: one partial record per workgroup.
//   k_diag_finish   one workgroup: thread t folds the partials t, t + T, ... in ascending order, then the same tree, and writes the row.
// An extremum travels as (value, index) and the lower index wins on equal values, so the pair is the same however the tree pairs the points up.
#include <math.h>

#include "pn_common.h"
#include "pn_sim_rhs.h"
#include "pn_sim_svd.h"

#define PN_DIAG_THREADS 256                          // four waves: one per SIMD, the SVD's fp64 registers to themselves (no second wave to share with)
#define PN_DIAG_IPS (PN_DIAG_THREADS / 8)            // points per workgroup = partial records per 32 points
#define PN_DIAG_FINISH_THREADS 256
#define PN_DIAG_NSUM 15                              // the row's 13 sums (mass, m x [3], P[3], L[3], kinetic, gravity, elastic) and its 2 counts
#define PN_DIAG_NEXT 5                               // sig_min, sig_max, det_min, strain_max, speed_max
#define PN_DIAG_MAX_IPS (1 << 27)                    // as pn_ip_state: p * 8 + i stays an int

static_assert(13 + 2 * PN_DIAG_NEXT + 2 == PN_DIAG_DOUBLES, "the row: 13 sums, 5 (value, index) pairs, 2 counts");
static_assert(PN_DIAG_THREADS % PN_WAVE == 0 && PN_DIAG_FINISH_THREADS % PN_WAVE == 0, "whole waves");

namespace {

// What a lane, a wave, a workgroup and the whole cloud carry: sums (the two counts ride along as doubles, exact below 2^53) and the extrema with
// their point; index < 0: no point yet.
struct DiagAcc {
    double s[PN_DIAG_NSUM];
    double ev[PN_DIAG_NEXT];
    int ei[PN_DIAG_NEXT];
};

__device__ __forceinline__ void diag_clear(DiagAcc& a) {
#pragma unroll
    for (int i = 0; i < PN_DIAG_NSUM; i++) a.s[i] = 0.0;
#pragma unroll
    for (int e = 0; e < PN_DIAG_NEXT; e++) { a.ev[e] = 0.0; a.ei[e] = -1; }
}

// extremum e is a maximum (sig_max, strain_max, speed_max) or a minimum (sig_min, det_min)
__device__ __forceinline__ constexpr bool diag_is_max(int e) { return e == 1 || e >= 3; }

// (v, i) <- the better of (v, i) and (bv, bi); on equal values the lower index.  Symmetric, so a tree may pair the points up in any way.
template <int E>
__device__ __forceinline__ void diag_take(double& v, int& i, double bv, int bi) {
    if (bi < 0) return;
    const bool better = i < 0 || (diag_is_max(E) ? bv > v : bv < v) || (bv == v && bi < i);
    if (better) { v = bv; i = bi; }
}

template <int E>
__device__ __forceinline__ void diag_wave_ext(DiagAcc& a) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double bv = __shfl_down(a.ev[E], off);
        const int bi = __shfl_down(a.ei[E], off);
        diag_take<E>(a.ev[E], a.ei[E], bv, bi);
    }
}

// lane 0 of the wave ends with the wave's record: the shuffle tree 32, 16 ... 1
__device__ __forceinline__ void diag_wave_reduce(DiagAcc& a) {
#pragma unroll
    for (int i = 0; i < PN_DIAG_NSUM; i++) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) a.s[i] += __shfl_down(a.s[i], off);
    }
    diag_wave_ext<0>(a); diag_wave_ext<1>(a); diag_wave_ext<2>(a); diag_wave_ext<3>(a); diag_wave_ext<4>(a);
}

template <int E>
__device__ __forceinline__ void diag_fold_ext(int e, int waves, const double (*sv)[PN_DIAG_NEXT], const int (*si)[PN_DIAG_NEXT], double& v, int& i) {
    if (e != E) return;
    for (int w = 0; w < waves; w++) diag_take<E>(v, i, sv[w][E], si[w][E]);
}

// The workgroup's record from its threads' records: the wave tree, then the waves in ascending order.  FINISH: the row (centre of mass divided out,
// NaN and -1 for an extremum no point entered); else a partial record in the row's layout with m x in the centre's place.
template <int THREADS, bool FINISH>
__device__ __forceinline__ void diag_block_write(DiagAcc& a, int t, double* __restrict__ out) {
    constexpr int WAVES = THREADS / PN_WAVE;
    __shared__ double s_sum[WAVES][PN_DIAG_NSUM];
    __shared__ double s_ev[WAVES][PN_DIAG_NEXT];
    __shared__ int s_ei[WAVES][PN_DIAG_NEXT];
    diag_wave_reduce(a);
    if ((t & (PN_WAVE - 1)) == 0) {
        const int w = t / PN_WAVE;
#pragma unroll
        for (int i = 0; i < PN_DIAG_NSUM; i++) s_sum[w][i] = a.s[i];
#pragma unroll
        for (int e = 0; e < PN_DIAG_NEXT; e++) { s_ev[w][e] = a.ev[e]; s_ei[w][e] = a.ei[e]; }
    }
    __syncthreads();
    if (t < PN_DIAG_NSUM) {
        double s = s_sum[0][t];
#pragma unroll
        for (int w = 1; w < WAVES; w++) s += s_sum[w][t];
        if (FINISH && t >= 1 && t <= 3) {   // com = sum m x / mass
            double m = s_sum[0][0];   // the mass, added as the thread that writes it adds it
#pragma unroll
            for (int w = 1; w < WAVES; w++) m += s_sum[w][0];
            s = m > 0.0 ? s / m : 0.0;
        }
        out[t < 13 ? t : t + 2 * PN_DIAG_NEXT] = s;   // the counts stand behind the extrema
    } else if (t < PN_DIAG_NSUM + PN_DIAG_NEXT) {
        const int e = t - PN_DIAG_NSUM;
        double v = 0.0;
        int i = -1;
        diag_fold_ext<0>(e, WAVES, s_ev, s_ei, v, i); diag_fold_ext<1>(e, WAVES, s_ev, s_ei, v, i); diag_fold_ext<2>(e, WAVES, s_ev, s_ei, v, i);
        diag_fold_ext<3>(e, WAVES, s_ev, s_ei, v, i); diag_fold_ext<4>(e, WAVES, s_ev, s_ei, v, i);
        out[13 + 2 * e] = (FINISH && i < 0) ? (double)NAN : v;
        out[13 + 2 * e + 1] = (double)i;
    }
}

__device__ __forceinline__ double diag_sum8(double v) {
    v += shfl_xor_d(v, 1);
    v += shfl_xor_d(v, 2);
    v += shfl_xor_d(v, 4);
    return v;
}

__device__ __forceinline__ bool diag_finite3(const double* a) { return isfinite(a[0]) && isfinite(a[1]) && isfinite(a[2]); }
__device__ __forceinline__ bool diag_finite9(const M3& a) { return diag_finite3(a.m[0]) && diag_finite3(a.m[1]) && diag_finite3(a.m[2]); }

}  // namespace

__global__ void __launch_bounds__(PN_DIAG_THREADS) k_diag_points(int n_k, int n_IP, double dx3, double dx5_12, double gx, double gy, double gz,
                                                                 const double* __restrict__ dof, const double* __restrict__ dof_vel,
                                                                 const int* __restrict__ topo, const double* __restrict__ rho,
                                                                 const double* __restrict__ mu, const double* __restrict__ lam,
                                                                 const double* __restrict__ Nx, const double* __restrict__ dNx,
                                                                 const double* __restrict__ ddNx, double* __restrict__ partial,
                                                                 double* __restrict__ per_point) {
    const int t = threadIdx.x, slot = t & 7;
    const int p_raw = blockIdx.x * PN_DIAG_IPS + (t >> 3);   // < n_IP + PN_DIAG_IPS <= 2^27 + 32
    const bool live = p_raw < n_IP;
    const int p = live ? p_raw : n_IP - 1;                   // a lane behind the last point computes that point again and enters nothing

    // position and velocity as every right-hand-side stage sees them; false: a kernel id out of range (never with the tables solver.py builds)
    double x[3], v[3];
    bool fin = pn_ip_state(p, n_k, dof, dof_vel, topo, Nx, x, v);

    int kid = topo[p * 8 + slot];
    kid = (unsigned)kid < (unsigned)n_k ? kid : 0;           // (fin is false then: the point is counted as non-finite, and no read leaves dof)
    const double* __restrict__ d = dof + (size_t)kid * 30;
    const double* __restrict__ dv = dof_vel + (size_t)kid * 30;
    const size_t ps = (size_t)p * 8 + slot;
    M3 F, G;
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) F.m[r][c] = G.m[r][c] = 0.0;
    ip_F_partial(d, dNx + ps * 30, F);
    ip_F_partial(dv, dNx + ps * 30, G);
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            F.m[r][c] = diag_sum8(F.m[r][c]);
            G.m[r][c] = diag_sum8(G.m[r][c]);
        }
    // H three components at a time: only |H|^2 (and whether all 27 are finite) outlives the loop
    double hh = 0.0;
#pragma unroll 1
    for (int r = 0; r < 9; r++) {
        double a[3] = {0.0, 0.0, 0.0};
        pn_ip_row_acc(d, ddNx + (ps * 9 + r) * 10, a[0], a[1], a[2]);
        a[0] = diag_sum8(a[0]); a[1] = diag_sum8(a[1]); a[2] = diag_sum8(a[2]);
        fin = fin && diag_finite3(a);
        hh += a[0] * a[0] + a[1] * a[1] + a[2] * a[2];
    }
    fin = fin && diag_finite3(x) && diag_finite3(v) && diag_finite9(F) && diag_finite9(G);

    const double m = rho[p] * dx3, j = rho[p] * dx5_12;
    const double NaN = (double)NAN;
    double ke = NaN, ee = NaN, ge = NaN, det = NaN, strain = NaN, speed = NaN, sig[3] = {NaN, NaN, NaN};
    double P[3] = {0.0, 0.0, 0.0}, L[3] = {0.0, 0.0, 0.0};
    if (fin) {   // (the same for a point's eight lanes; no shuffle inside)
        M3 U, V;
        svd3(F, U, sig, V);
        double sp[3];
        volume_invariant_project(sig, sp);
        det = det33(F);
        const double mu_p = mu[p], lam_p = lam[p];
        double e1 = 0.0, e2 = 0.0, gg = 0.0;
#pragma unroll
        for (int i = 0; i < 3; i++) {
            e1 += (sig[i] - 1.0) * (sig[i] - 1.0);
            e2 += (sig[i] - sp[i]) * (sig[i] - sp[i]);
        }
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int c = 0; c < 3; c++) gg += G.m[r][c] * G.m[r][c];
        const double vv = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
        ke = 0.5 * m * vv + 0.5 * j * gg;
        ee = dx3 * (0.5 * mu_p * e1 + 0.5 * lam_p * e2) + dx5_12 * (0.5 * (mu_p + lam_p)) * hh;
        ge = -m * (gx * x[0] + gy * x[1] + gz * x[2]);
        strain = sqrt(e1);
        speed = sqrt(vv);
        double fxg[3] = {0.0, 0.0, 0.0};   // sum over columns c of F[:,c] x G[:,c]
#pragma unroll
        for (int c = 0; c < 3; c++) {
            fxg[0] += F.m[1][c] * G.m[2][c] - F.m[2][c] * G.m[1][c];
            fxg[1] += F.m[2][c] * G.m[0][c] - F.m[0][c] * G.m[2][c];
            fxg[2] += F.m[0][c] * G.m[1][c] - F.m[1][c] * G.m[0][c];
        }
        L[0] = m * (x[1] * v[2] - x[2] * v[1]) + j * fxg[0];
        L[1] = m * (x[2] * v[0] - x[0] * v[2]) + j * fxg[1];
        L[2] = m * (x[0] * v[1] - x[1] * v[0]) + j * fxg[2];
        P[0] = m * v[0]; P[1] = m * v[1]; P[2] = m * v[2];
    }

    if (per_point && live) {   // (m, ke, ee, det, sig0, sig1, sig2, strain): a point's lane `slot` writes entry `slot`, 512 contiguous bytes per wave
        const double rec = slot == 0 ? m : slot == 1 ? ke : slot == 2 ? ee : slot == 3 ? det : slot == 4 ? sig[0] : slot == 5 ? sig[1] : slot == 6 ? sig[2] : strain;
        per_point[(size_t)p * 8 + slot] = rec;
    }

    DiagAcc a;
    diag_clear(a);
    if (live && slot == 0) {
        if (fin) {
            a.s[0] = m;
            a.s[1] = m * x[0]; a.s[2] = m * x[1]; a.s[3] = m * x[2];
            a.s[4] = P[0]; a.s[5] = P[1]; a.s[6] = P[2];
            a.s[7] = L[0]; a.s[8] = L[1]; a.s[9] = L[2];
            a.s[10] = ke; a.s[11] = ge; a.s[12] = ee;
            a.s[14] = det <= 0.0 ? 1.0 : 0.0;
            a.ev[0] = sig[2]; a.ev[1] = sig[0]; a.ev[2] = det; a.ev[3] = strain; a.ev[4] = speed;
#pragma unroll
            for (int e = 0; e < PN_DIAG_NEXT; e++) a.ei[e] = p;
        } else {
            a.s[13] = 1.0;
        }
    }
    diag_block_write<PN_DIAG_THREADS, false>(a, t, partial + (size_t)blockIdx.x * PN_DIAG_DOUBLES);
}

template <int E>
__device__ __forceinline__ void diag_take_partial(DiagAcc& a, const double* __restrict__ r) {
    diag_take<E>(a.ev[E], a.ei[E], r[13 + 2 * E], (int)r[13 + 2 * E + 1]);
}

__global__ void __launch_bounds__(PN_DIAG_FINISH_THREADS) k_diag_finish(int n_part, const double* __restrict__ partial, double* __restrict__ row) {
    const int t = threadIdx.x;
    DiagAcc a;
    diag_clear(a);
    for (int q = t; q < n_part; q += PN_DIAG_FINISH_THREADS) {
        const double* __restrict__ r = partial + (size_t)q * PN_DIAG_DOUBLES;
#pragma unroll
        for (int i = 0; i < PN_DIAG_NSUM; i++) a.s[i] += r[i < 13 ? i : i + 2 * PN_DIAG_NEXT];
        diag_take_partial<0>(a, r); diag_take_partial<1>(a, r); diag_take_partial<2>(a, r); diag_take_partial<3>(a, r); diag_take_partial<4>(a, r);
    }
    diag_block_write<PN_DIAG_FINISH_THREADS, true>(a, t, row);
}

extern "C" int pn_sim_diagnostics_doubles(void) { return PN_DIAG_DOUBLES; }

extern "C" uint64_t pn_sim_diagnostics_work_doubles(int n_IP) {
    return n_IP > 0 ? (uint64_t)pn_div_up((uint64_t)n_IP, PN_DIAG_IPS) * PN_DIAG_DOUBLES : 0;
}

extern "C" int pn_sim_diagnostics(int n_k, int n_IP, double dx, const double* g3_host, const double* dof, const double* dof_vel, const int* topo,
                                  const double* rho, const double* mu, const double* lam, const double* Nx, const double* dNx, const double* ddNx,
                                  double* work, double* row_out, double* per_point, void* stream) {
    PN_REQUIRE(n_k > 0 && n_IP > 0 && n_IP <= PN_DIAG_MAX_IPS);
    PN_REQUIRE(isfinite(dx) && dx > 0.0);
    PN_REQUIRE(g3_host && dof && dof_vel && topo && rho && mu && lam && Nx && dNx && ddNx && work && row_out);
    const int n_part = (int)pn_div_up((uint64_t)n_IP, PN_DIAG_IPS);
    const double dx3 = dx * dx * dx;
    hipStream_t s = (hipStream_t)stream;
    k_diag_points<<<n_part, PN_DIAG_THREADS, 0, s>>>(n_k, n_IP, dx3, dx3 * dx * dx / 12.0, g3_host[0], g3_host[1], g3_host[2], dof, dof_vel, topo, rho,
                                                     mu, lam, Nx, dNx, ddNx, work, per_point);
    PN_LAUNCH_CHECK();
    k_diag_finish<<<1, PN_DIAG_FINISH_THREADS, 0, s>>>(n_part, work, row_out);
    PN_LAUNCH_CHECK();
    return PN_OK;
}
