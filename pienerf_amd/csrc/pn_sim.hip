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
#include <math.h>

#include <vector>

#include "pn_common.h"
#include "pn_sim_ip.h"

// The substep is a chain of ~30 short dependent launches that runs concurrently with the render kernels of other frames
// (harness.capture_pipelined): its waves ask the SIMD arbiter for the highest user priority so the chain's latency does not
// stretch when the CUs are full of march waves.
#ifndef PN_SIM_PRIO_LEVEL
#define PN_SIM_PRIO_LEVEL 3
#endif
#define PN_SIM_PRIO() __builtin_amdgcn_s_setprio(PN_SIM_PRIO_LEVEL)

namespace {

struct M3 { double m[3][3]; };

__device__ __forceinline__ M3 mul33(const M3& a, const M3& b) {
    M3 c;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) c.m[i][j] = a.m[i][0] * b.m[0][j] + a.m[i][1] * b.m[1][j] + a.m[i][2] * b.m[2][j];
    return c;
}
__device__ __forceinline__ double det33(const M3& a) {
    return a.m[0][0] * (a.m[1][1] * a.m[2][2] - a.m[1][2] * a.m[2][1]) - a.m[0][1] * (a.m[1][0] * a.m[2][2] - a.m[1][2] * a.m[2][0]) +
           a.m[0][2] * (a.m[1][0] * a.m[2][1] - a.m[1][1] * a.m[2][0]);
}

// v_rcp_f64 / v_rsq_f64 (~26 good bits) + two Newton steps: ~1 ulp, a third of the dependent-instruction count of the IEEE
// divide / sqrt expansions.  The SVD below is one long fp64 dependency chain per IP (k_elastic is latency-bound on it), and its
// results are compared with the oracle by tolerance, not bit for bit.
__device__ __forceinline__ double fast_rcp(double x) {
    double r = __builtin_amdgcn_rcp(x);
    r = fma(fma(-x, r, 1.0), r, r);
    return fma(fma(-x, r, 1.0), r, r);
}
__device__ __forceinline__ double fast_rsq(double x) {
    double y = __builtin_amdgcn_rsq(x);
    double e = fma(-x * y, y, 1.0);
    y = fma(0.5 * y, e, y);
    e = fma(-x * y, y, 1.0);
    return fma(0.5 * y, e, y);
}

// One Jacobi rotation zeroing S[p][q] of the symmetric S, accumulated into Q (columns = eigenvectors).
// skip > 0 (threshold Jacobi): a pair whose off-diagonal is already below sqrt(skip) of its diagonal entries is left alone — its rotation would move
// nothing above that level, and in the late sweeps of a warm-started decomposition that is most pairs (~100 dependent instructions each).
template <int p, int q>
__device__ __forceinline__ void jacobi_rot(M3& S, M3& Q, double skip = 0.0) {
    const double spq = S.m[p][q];
    if (spq * spq <= skip * fabs(S.m[p][p] * S.m[q][q])) return;   // (skip == 0: spq == 0)
    const double theta = (S.m[q][q] - S.m[p][p]) * fast_rcp(2.0 * spq);
    double t;
    if (fabs(theta) > 1e100) {
        t = 0.5 * fast_rcp(theta);  // theta^2 would overflow; t = 1 / (2 theta) to full precision there
    } else {
        const double h = fma(theta, theta, 1.0);
        t = (theta >= 0 ? 1.0 : -1.0) * fast_rcp(fabs(theta) + h * fast_rsq(h));
    }
    const double c = fast_rsq(fma(t, t, 1.0)), s = t * c;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double a = S.m[k][p], b = S.m[k][q];
        S.m[k][p] = c * a - s * b;
        S.m[k][q] = s * a + c * b;
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double a = S.m[p][k], b = S.m[q][k];
        S.m[p][k] = c * a - s * b;
        S.m[q][k] = s * a + c * b;
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double a = Q.m[k][p], b = Q.m[k][q];
        Q.m[k][p] = c * a - s * b;
        Q.m[k][q] = s * a + c * b;
    }
}

// F = U diag(sig) V^T with det U = det V = +1, |sig| descending, sig[2] signed (contract of wp.svd3, cuda_utils.py:107).
// Q0 (may be null): a rotation to start the Jacobi iteration from — the V of the same integration point one local/global iteration earlier.
// F changes by ~1e-3 between iterations, so Q0^T (F^T F) Q0 is already diagonal to ~1e-6 and two sweeps finish what five do from the identity
// (the chain below is what k_elastic's duration consists of: 8 of its 15 us).  The decomposition is the same up to rounding: R = U V^T and
// U diag(s') V^T do not depend on where the iteration started.  tol: stop at off^2 <= tol dia^2.
__device__ void svd3(const M3& F, M3& U, double* sig, M3& V, const M3* Q0 = nullptr, double tol = 1e-30, double skip = 0.0) {
    M3 S, Q;
    if (Q0) {
        const M3 B0 = mul33(F, *Q0);  // S = (F Q0)^T (F Q0)
        Q = *Q0;
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) S.m[i][j] = B0.m[0][i] * B0.m[0][j] + B0.m[1][i] * B0.m[1][j] + B0.m[2][i] * B0.m[2][j];
    } else {
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) {
                S.m[i][j] = F.m[0][i] * F.m[0][j] + F.m[1][i] * F.m[1][j] + F.m[2][i] * F.m[2][j];
                Q.m[i][j] = (i == j) ? 1.0 : 0.0;
            }
    }
    for (int sweep = 0; sweep < 32; sweep++) {
        const double off = S.m[0][1] * S.m[0][1] + S.m[0][2] * S.m[0][2] + S.m[1][2] * S.m[1][2];
        const double dia = S.m[0][0] * S.m[0][0] + S.m[1][1] * S.m[1][1] + S.m[2][2] * S.m[2][2];
        // fp64 rounding leaves off ~ 1e-32 dia however long one sweeps (a 1e-34 test never fires and all 32 sweeps run);
        // 1e-30 is reached one sweep after ~1e-15 (quadratic convergence) — same rule as the oracle
        if (off <= tol * dia || off == 0.0) break;
        jacobi_rot<0, 1>(S, Q, skip);
        jacobi_rot<0, 2>(S, Q, skip);
        jacobi_rot<1, 2>(S, Q, skip);
    }
    M3 B = mul33(F, Q);
    double n0 = B.m[0][0] * B.m[0][0] + B.m[1][0] * B.m[1][0] + B.m[2][0] * B.m[2][0];
    double n1 = B.m[0][1] * B.m[0][1] + B.m[1][1] * B.m[1][1] + B.m[2][1] * B.m[2][1];
    double n2 = B.m[0][2] * B.m[0][2] + B.m[1][2] * B.m[1][2] + B.m[2][2] * B.m[2][2];
    // sort columns by descending norm with explicit swaps (each swap flips det; fixed afterwards)
    auto swapc = [&](int a, int b) {
#pragma unroll
        for (int i = 0; i < 3; i++) {
            double t = B.m[i][a]; B.m[i][a] = B.m[i][b]; B.m[i][b] = t;
            t = Q.m[i][a]; Q.m[i][a] = Q.m[i][b]; Q.m[i][b] = t;
        }
    };
    if (n0 < n1) { swapc(0, 1); double t = n0; n0 = n1; n1 = t; }
    if (n0 < n2) { swapc(0, 2); double t = n0; n0 = n2; n2 = t; }
    if (n1 < n2) { swapc(1, 2); double t = n1; n1 = n2; n2 = t; }
    if (det33(Q) < 0) {
#pragma unroll
        for (int i = 0; i < 3; i++) { Q.m[i][2] = -Q.m[i][2]; B.m[i][2] = -B.m[i][2]; }
    }
    double u0[3], u1[3], u2[3];
    double l0 = 0.0;
    if (n0 > 0) {
        const double il0 = fast_rsq(n0);
        l0 = n0 * il0;
        u0[0] = B.m[0][0] * il0; u0[1] = B.m[1][0] * il0; u0[2] = B.m[2][0] * il0;
    } else { u0[0] = 1; u0[1] = 0; u0[2] = 0; }
    const double d01 = u0[0] * B.m[0][1] + u0[1] * B.m[1][1] + u0[2] * B.m[2][1];
#pragma unroll
    for (int i = 0; i < 3; i++) u1[i] = B.m[i][1] - d01 * u0[i];
    const double q1 = u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2];
    double l1 = 0.0, il1 = 0.0;
    if (q1 > 1e-290) { il1 = fast_rsq(q1); l1 = q1 * il1; }
    if (l1 > 1e-300 && l1 > 1e-14 * l0) {
#pragma unroll
        for (int i = 0; i < 3; i++) u1[i] *= il1;
    } else {  // rank <= 1: any unit vector orthogonal to u0
        const double a0 = fabs(u0[0]), a1 = fabs(u0[1]), a2 = fabs(u0[2]);
        const int k = a0 < a1 ? (a0 < a2 ? 0 : 2) : (a1 < a2 ? 1 : 2);
        const double d = (k == 0) ? u0[0] : (k == 1 ? u0[1] : u0[2]);
#pragma unroll
        for (int i = 0; i < 3; i++) u1[i] = ((i == k) ? 1.0 : 0.0) - d * u0[i];
        l1 = sqrt(u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2]);
#pragma unroll
        for (int i = 0; i < 3; i++) u1[i] /= l1;
    }
    u2[0] = u0[1] * u1[2] - u0[2] * u1[1];
    u2[1] = u0[2] * u1[0] - u0[0] * u1[2];
    u2[2] = u0[0] * u1[1] - u0[1] * u1[0];
#pragma unroll
    for (int i = 0; i < 3; i++) { U.m[i][0] = u0[i]; U.m[i][1] = u1[i]; U.m[i][2] = u2[i]; }
    V = Q;
#pragma unroll
    for (int j = 0; j < 3; j++) sig[j] = U.m[0][j] * B.m[0][j] + U.m[1][j] * B.m[1][j] + U.m[2][j] * B.m[2][j];
}

// ------------------------------------------------------------------------------------------------ svd3, the published algorithm (PN_SIM_SVD=mcadams)
// wp.svd3 (cuda_utils.py:107; warp-lang is absent from /root/reference) implements McAdams, Selle, Tamstorf, Teran, Sifakis, "Computing the
// Singular Value Decomposition of 3x3 matrices with minimal branching and elementary floating point operations" (UW-Madison TR1690): a FIXED
// number of cyclic Jacobi sweeps on F^T F with the approximate Givens quaternion (TR section 2), singular values ordered by conditional
// negating swaps (section 3), U and the diagonal from a Givens-quaternion QR of F V (section 4).  The default decomposition above runs to
// convergence instead; this one exists so that the simulator can be run ON the reference's algorithm, sweep count included: with 8 sweeps the two
// agree to 2e-7 of the displacements (the paper's 10-digit constants), with 4 sweeps — the paper's single-precision setting — they differ by
// 2.6e-4 on the chair (tests/test_oracle_svd.py), which is above the 1e-4 bar: which sweep count the reference's build runs with decides
// which of the two it is closer to, and both are here.  Same arithmetic as the test suite's CPU restatement of the algorithm (IEEE divide / sqrt, no
// warm start, no early exit), compared with it at 1e-10 (tests/test_gpu_simpin.py).
struct Quat4 { double x, y, z, w; };
__device__ __forceinline__ Quat4 qmul4(const Quat4& a, const Quat4& b) {
    return {a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y, a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x,
            a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w, a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z};
}
__device__ __forceinline__ void quat_to_m3(const Quat4& q, M3& r) {
    const double xx = q.x * q.x, yy = q.y * q.y, zz = q.z * q.z, xy = q.x * q.y, xz = q.x * q.z, yz = q.y * q.z, wx = q.w * q.x, wy = q.w * q.y, wz = q.w * q.z;
    r.m[0][0] = 1 - 2 * (yy + zz); r.m[0][1] = 2 * (xy - wz);     r.m[0][2] = 2 * (xz + wy);
    r.m[1][0] = 2 * (xy + wz);     r.m[1][1] = 1 - 2 * (xx + zz); r.m[1][2] = 2 * (yz - wx);
    r.m[2][0] = 2 * (xz - wy);     r.m[2][1] = 2 * (yz + wx);     r.m[2][2] = 1 - 2 * (xx + yy);
}
// one conjugation S <- G^T S G in the plane (P, Q), the rotation's half-angle quaternion multiplied onto q (axis AX = 3 - P - Q)
template <int P, int Q, int AX>
__device__ __forceinline__ void mc_conjugate(M3& S, Quat4& q) {
    double ch = 2.0 * (S.m[P][P] - S.m[Q][Q]), sh = S.m[P][Q];
    const bool ok = 5.828427124 * sh * sh < ch * ch;                 // gamma = 3 + 2 sqrt 2, cos / sin(pi / 8): the paper's digits
    const double w = 1.0 / sqrt(ch * ch + sh * sh);
    ch = ok ? w * ch : 0.923879532;
    sh = ok ? w * sh : 0.3826834323;
    const double scale = ch * ch + sh * sh, c = (ch * ch - sh * sh) / scale, s = (2.0 * sh * ch) / scale;
    M3 T = S;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        T.m[i][P] = c * S.m[i][P] + s * S.m[i][Q];
        T.m[i][Q] = -s * S.m[i][P] + c * S.m[i][Q];
    }
    M3 R = T;
#pragma unroll
    for (int j = 0; j < 3; j++) {
        R.m[P][j] = c * T.m[P][j] + s * T.m[Q][j];
        R.m[Q][j] = -s * T.m[P][j] + c * T.m[Q][j];
    }
    R.m[P][Q] = R.m[Q][P] = 0.5 * (R.m[P][Q] + R.m[Q][P]);
    S = R;
    Quat4 g{0, 0, 0, ch};
    (AX == 0 ? g.x : AX == 1 ? g.y : g.z) = sh;
    q = qmul4(q, g);
}
__device__ __forceinline__ void mc_qr_givens(double piv, double low, double eps, double& ch, double& sh) {
    const double r2 = piv * piv + low * low;
    const double rho = r2 > 0 ? r2 * (1.0 / sqrt(r2)) : 0.0;
    sh = rho > eps ? low : 0.0;
    ch = fabs(piv) + fmax(rho, eps);
    if (piv < 0) { const double t = sh; sh = ch; ch = t; }
    const double w = 1.0 / sqrt(ch * ch + sh * sh);
    ch *= w;
    sh *= w;
}
template <int A, int B_>
__device__ __forceinline__ void mc_rot_rows(M3& B, double ch, double sh) {
    const double c = 1.0 - 2.0 * sh * sh, s = 2.0 * ch * sh;
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const double x = B.m[A][j], y = B.m[B_][j];
        B.m[A][j] = c * x + s * y;
        B.m[B_][j] = -s * x + c * y;
    }
}
__device__ void svd3_mcadams(const M3& F, M3& U, double* sig, M3& V, int sweeps) {
    M3 S;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) S.m[i][j] = F.m[0][i] * F.m[0][j] + F.m[1][i] * F.m[1][j] + F.m[2][i] * F.m[2][j];
    Quat4 q{0, 0, 0, 1};
    for (int sweep = 0; sweep < sweeps; sweep++) {
        mc_conjugate<0, 1, 2>(S, q);
        mc_conjugate<1, 2, 0>(S, q);
        mc_conjugate<2, 0, 1>(S, q);
    }
    quat_to_m3(q, V);
    M3 B = mul33(F, V);
    double rho[3];
#pragma unroll
    for (int j = 0; j < 3; j++) rho[j] = B.m[0][j] * B.m[0][j] + B.m[1][j] * B.m[1][j] + B.m[2][j] * B.m[2][j];
    auto negswap = [&](int a, int b) {
        if (!(rho[a] < rho[b])) return;
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const double ba = B.m[i][a], va = V.m[i][a];
            B.m[i][a] = B.m[i][b]; B.m[i][b] = -ba;
            V.m[i][a] = V.m[i][b]; V.m[i][b] = -va;
        }
        const double t = rho[a]; rho[a] = rho[b]; rho[b] = t;
    };
    negswap(0, 1);
    negswap(0, 2);
    negswap(1, 2);
    double ch1, sh1, ch2, sh2, ch3, sh3;
    mc_qr_givens(B.m[0][0], B.m[1][0], 1e-12, ch1, sh1);
    mc_rot_rows<0, 1>(B, ch1, sh1);
    mc_qr_givens(B.m[0][0], B.m[2][0], 1e-12, ch2, sh2);
    mc_rot_rows<0, 2>(B, ch2, sh2);
    mc_qr_givens(B.m[1][1], B.m[2][1], 1e-12, ch3, sh3);
    mc_rot_rows<1, 2>(B, ch3, sh3);
    quat_to_m3(qmul4(qmul4(Quat4{0, 0, sh1, ch1}, Quat4{0, -sh2, 0, ch2}), Quat4{sh3, 0, 0, ch3}), U);
    sig[0] = B.m[0][0]; sig[1] = B.m[1][1]; sig[2] = B.m[2][2];
}

// simulator/func_utils.py:21-40
__device__ __forceinline__ void volume_invariant_project(const double* sig, double* out) {
    double D0 = 0, D1 = 0, D2 = 0;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const double a = sig[0] + D0, b = sig[1] + D1, c = sig[2] + D2;
        const double C = a * b * c - 1.0;
        const double g0 = b * c, g1 = a * c, g2 = a * b;
        const double coef = ((g0 * D0 + g1 * D1 + g2 * D2) - C) * fast_rcp(g0 * g0 + g1 * g1 + g2 * g2);
        D0 = coef * g0; D1 = coef * g1; D2 = coef * g2;
    }
    out[0] = sig[0] + D0; out[1] = sig[1] + D1; out[2] = sig[2] + D2;
}

__device__ __forceinline__ double shfl_xor_d(double v, int m) {
    int2 t = *reinterpret_cast<int2*>(&v);
    t.x = __shfl_xor(t.x, m);
    t.y = __shfl_xor(t.y, m);
    return *reinterpret_cast<double*>(&t);
}

}  // namespace

// mcadams_sweeps, the argument of every entry that runs calc_elastic: which svd3 its kernels run.  0 = the converged, warm-started threshold Jacobi
// (default); 1..64 = McAdams' algorithm with that many sweeps (PN_SIM_SVD=mcadams[:n] on the Python side); anything else is PN_ERR_ARG.
static inline bool pn_svd_sweeps_ok(int mcadams_sweeps) { return mcadams_sweeps >= 0 && mcadams_sweeps <= 64; }

#ifndef PN_SIM_STAMPS
#define PN_SIM_STAMPS 0
#endif
#if PN_SIM_STAMPS
// Timing build (tools/build_variant.py -DPN_SIM_STAMPS=1 with PN_VARIANT_UNITS=pn_sim.hip): the first thread of every substep kernel notes when its launch
// STARTED (100 MHz wall clock) and which kernel it is, into a ring a tool reads back (pn_sim_stamps_read): start-to-start gaps along the simulator's
// chain of dependent launches — alone, and beside the render lanes.  [0]: next slot; then entries (kernel id << 56 | ticks)
#define PN_SIM_STAMP_CAP 65536
__device__ unsigned long long g_sim_stamps[1 + PN_SIM_STAMP_CAP];
__device__ __forceinline__ void sim_stamp(int id) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const unsigned long long i = atomicAdd(&g_sim_stamps[0], 1ull);
        g_sim_stamps[1 + (i % PN_SIM_STAMP_CAP)] = ((unsigned long long)id << 56) | (__builtin_amdgcn_s_memrealtime() & 0x00ffffffffffffffull);
    }
}
extern "C" int pn_sim_stamps_read(unsigned long long* host, int reset) {
    PN_HIP_CHECK(hipDeviceSynchronize());
    if (host) PN_HIP_CHECK(hipMemcpyFromSymbol(host, HIP_SYMBOL(g_sim_stamps), sizeof(unsigned long long) * (1 + PN_SIM_STAMP_CAP)));
    if (reset) { const unsigned long long z = 0; PN_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_sim_stamps), &z, sizeof(z))); }
    return PN_OK;
}
#define PN_SIM_STAMP(id) sim_stamp(id)
// ... and phase clocks inside k_cells_elastic_gather: thread 0 of EVERY workgroup reads the 100 MHz clock at the phase boundaries (a scalar instruction,
// nothing in flight) and adds its differences to g_sim_phase at the very end: [p] ticks from boundary p to p + 1 summed over workgroups, [8] workgroups,
// [9] the largest start-to-end of a workgroup, [10 + p] the largest single difference
__device__ unsigned long long g_sim_phase[24];
#define PN_SIM_PHASE_DECL unsigned long long ph_[8]; int ph_n_ = 0
#define PN_SIM_PHASE_MARK do { if (ph_n_ < 8) ph_[ph_n_++] = __builtin_amdgcn_s_memrealtime(); } while (0)
__device__ __forceinline__ void sim_phase_flush(const unsigned long long* ph, int n) {
    if (threadIdx.x == 0) {
        for (int p = 0; p + 1 < n; p++) { atomicAdd(&g_sim_phase[p], ph[p + 1] - ph[p]); atomicMax(&g_sim_phase[10 + p], ph[p + 1] - ph[p]); }
        atomicAdd(&g_sim_phase[8], 1ull);
        atomicMax(&g_sim_phase[9], ph[n - 1] - ph[0]);
    }
}
extern "C" int pn_sim_phase_read(unsigned long long* host, int reset) {
    PN_HIP_CHECK(hipDeviceSynchronize());
    if (host) PN_HIP_CHECK(hipMemcpyFromSymbol(host, HIP_SYMBOL(g_sim_phase), sizeof(unsigned long long) * 24));
    if (reset) { unsigned long long z[24] = {0}; PN_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_sim_phase), z, sizeof(z))); }
    return PN_OK;
}
#define PN_SIM_PHASE(id) PN_SIM_PHASE_MARK
#define PN_SIM_PHASE_FLUSH sim_phase_flush(ph_, ph_n_)
#else
#define PN_SIM_STAMP(id)
#define PN_SIM_PHASE(id)
#define PN_SIM_PHASE_DECL
#define PN_SIM_PHASE_FLUSH
#endif

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

// ------------------------------------------------------------------------------------------------ calc_elastic
// 8 lanes per IP.  Writes RF/VF/FF (op-level, any may be NULL) and/or P = dx^3 (mu R + lam V) (step driver).
template <bool MC = false>
__global__ void __launch_bounds__(256) k_elastic(int n_IP, const int* __restrict__ topo, const double* __restrict__ dNx, const double* __restrict__ dof,
                                                 double* __restrict__ RF, double* __restrict__ VF, double* __restrict__ FF, double* __restrict__ P,
                                                 const double* __restrict__ mu, const double* __restrict__ lam, double dx3,
                                                 const int* __restrict__ csr_pos = nullptr, double* __restrict__ P_csr = nullptr,
                                                 double* __restrict__ Vstore = nullptr, int mc_sweeps = 0) {
    PN_SIM_STAMP(1);
    PN_SIM_PRIO();
    const int tid = threadIdx.x + blockIdx.x * blockDim.x;
    const int v = tid >> 3, i = tid & 7;
    const bool live = v < n_IP;
    M3 Fm;
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) Fm.m[r][c] = 0.0;
    if (live) {
        const int kid = topo[v * 8 + i];
        const double* __restrict__ d = dof + (size_t)kid * 30;
        const double* __restrict__ dn = dNx + ((size_t)v * 8 + i) * 30;
#pragma unroll
        for (int x = 0; x < 10; x++) {
            const double d0 = d[x * 3], d1 = d[x * 3 + 1], d2 = d[x * 3 + 2];
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const double g = dn[c * 10 + x];
                Fm.m[0][c] += d0 * g;
                Fm.m[1][c] += d1 * g;
                Fm.m[2][c] += d2 * g;
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            double s = Fm.m[r][c];
            s += shfl_xor_d(s, 1);
            s += shfl_xor_d(s, 2);
            s += shfl_xor_d(s, 4);
            Fm.m[r][c] = s;
        }
    if (!live) return;  // the 8 lanes of an IP share v: whole groups leave together
    double Pm[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (i == 0) {
        M3 U, V;
        double sig[3], sp[3];
        if (MC) {
            svd3_mcadams(Fm, U, sig, V, mc_sweeps);   // the published algorithm: fixed sweeps, no warm start
        } else if (Vstore) {
            // step driver: start from this IP's V of the previous local/global iteration (identity before the first substep), leave the new one.
            // 1e-24: off-diagonals below 1e-12 of the diagonal, ten digits beyond the 1e-4 relative bar of the DOF displacements
            M3 Q0;
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int c = 0; c < 3; c++) Q0.m[r][c] = Vstore[(size_t)v * 9 + r * 3 + c];
            svd3(Fm, U, sig, V, &Q0, 1e-24);
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int c = 0; c < 3; c++) Vstore[(size_t)v * 9 + r * 3 + c] = V.m[r][c];
        } else
        svd3(Fm, U, sig, V);
        volume_invariant_project(sig, sp);
        const double m_ = mu ? mu[v] : 0.0, l_ = lam ? lam[v] : 0.0;
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const double R = U.m[r][0] * V.m[c][0] + U.m[r][1] * V.m[c][1] + U.m[r][2] * V.m[c][2];
                const double Vv = U.m[r][0] * sp[0] * V.m[c][0] + U.m[r][1] * sp[1] * V.m[c][1] + U.m[r][2] * sp[2] * V.m[c][2];
                if (RF) RF[(size_t)v * 9 + r * 3 + c] = R;
                if (VF) VF[(size_t)v * 9 + r * 3 + c] = Vv;
                if (FF) FF[(size_t)v * 9 + r * 3 + c] = U.m[r][0] * sig[0] * V.m[c][0] + U.m[r][1] * sig[1] * V.m[c][1] + U.m[r][2] * sig[2] * V.m[c][2];
                Pm[r * 3 + c] = dx3 * (m_ * R + l_ * Vv);
                if (P) P[(size_t)v * 9 + r * 3 + c] = Pm[r * 3 + c];
            }
    }
    if (P_csr) {
        // step driver: P also goes, once per neighbour slot, to that slot's position in its kernel's CSR list, so that the
        // gather (k_rhs_gather_csr) reads P and dNx as two contiguous streams with no index to chase
        const int src = (threadIdx.x & 63) & ~7;
        double* __restrict__ dst = P_csr + (size_t)csr_pos[v * 8 + i] * 9;
#pragma unroll
        for (int q = 0; q < 9; q++) {
            int2 t = *reinterpret_cast<int2*>(&Pm[q]);
            t.x = __shfl(t.x, src);
            t.y = __shfl(t.y, src);
            dst[q] = *reinterpret_cast<double*>(&t);
        }
    }
}

extern "C" int pn_sim_calc_elastic(int n_IP, const int* topo, const double* dNx, const double* dof, double* RF, double* VF, double* FF,
                                   int mcadams_sweeps, void* stream) {
    PN_REQUIRE(n_IP > 0 && topo && dNx && dof && RF && VF && pn_svd_sweeps_ok(mcadams_sweeps));
    if (mcadams_sweeps)
        k_elastic<true><<<pn_div_up((uint64_t)n_IP * 8, 256), 256, 0, (hipStream_t)stream>>>(n_IP, topo, dNx, dof, RF, VF, FF, nullptr, nullptr, nullptr, 0.0,
                                                                                             nullptr, nullptr, nullptr, mcadams_sweeps);
    else
        k_elastic<false><<<pn_div_up((uint64_t)n_IP * 8, 256), 256, 0, (hipStream_t)stream>>>(n_IP, topo, dNx, dof, RF, VF, FF, nullptr, nullptr, nullptr, 0.0);
    PN_LAUNCH_CHECK();
    return PN_OK;
}

// ------------------------------------------------------------------------------------------------ collect_rhs (gather form)
// One wave per kernel k.  Entry e of the CSR list = vid*8 + dir.  Lane-strided accumulation of the 10x3 block, fixed
// xor-tree reduction.  mode 0: rhs = sum (P from mu/lam/RF/VF); mode 1 (step driver): out = momentum + sum - rhs_rest.
__global__ void __launch_bounds__(256) k_rhs_gather(int n_k, double dx3, const int* __restrict__ csr_bg, const int* __restrict__ csr_cnt,
                                                    const int* __restrict__ csr_buf, const double* __restrict__ mu, const double* __restrict__ lam,
                                                    const double* __restrict__ dNx, const double* __restrict__ RF, const double* __restrict__ VF,
                                                    const double* __restrict__ P, const double* __restrict__ momentum,
                                                    const double* __restrict__ rhs_rest, double* __restrict__ out) {
    PN_SIM_PRIO();
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= n_k) return;
    const int lane = threadIdx.x & 63;
    double acc[30];
#pragma unroll
    for (int q = 0; q < 30; q++) acc[q] = 0.0;
    const int bg = csr_bg[k], cnt = csr_cnt[k];
    for (int e = lane; e < cnt; e += 64) {
        const int code = csr_buf[bg + e];
        const int v = code >> 3;
        double Pm[9];
        if (P) {
#pragma unroll
            for (int q = 0; q < 9; q++) Pm[q] = P[(size_t)v * 9 + q];
        } else {
            const double m_ = mu[v], l_ = lam[v];
#pragma unroll
            for (int q = 0; q < 9; q++) Pm[q] = dx3 * (m_ * RF[(size_t)v * 9 + q] + l_ * VF[(size_t)v * 9 + q]);
        }
        const double* __restrict__ dn = dNx + (size_t)code * 30;  // [c][x]
#pragma unroll
        for (int x = 0; x < 10; x++) {
            const double g0 = dn[x], g1 = dn[10 + x], g2 = dn[20 + x];
#pragma unroll
            for (int r = 0; r < 3; r++) acc[x * 3 + r] += Pm[r * 3] * g0 + Pm[r * 3 + 1] * g1 + Pm[r * 3 + 2] * g2;
        }
    }
#pragma unroll
    for (int q = 0; q < 30; q++) {
        double s = acc[q];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += shfl_xor_d(s, o);
        acc[q] = s;
    }
    if (lane < 30) {
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < 30; q++) if (q == lane) s = acc[q];
        const size_t o = (size_t)k * 30 + lane;
        out[o] = momentum ? (momentum[o] + s - rhs_rest[o]) : s;
    }
}

// Step-driver form of the gather: one 1024-thread workgroup per kernel over CSR-ORDERED copies of dNx (dNx_csr[entry][c][x],
// built once at initialisation) and, when calc_elastic wrote it, of P (P_csr[entry][r][c]): the 240 B + 72 B of every entry are
// read as contiguous streams with no index to follow.  Thread (slot, q = c*10 + x) walks entries slot, slot+32, ... and
// accumulates the three rows r of P[r][c] * dNx[c][x]; the 32 slots x 3 columns c are then reduced through LDS in a fixed
// order (bit-reproducible run to run).  out = momentum + sum - rhs_rest.
#define PN_GATHER_SLOTS 32
__global__ void __launch_bounds__(1024) k_rhs_gather_csr(int n_k, const int* __restrict__ csr_bg, const int* __restrict__ csr_cnt,
                                                         const int* __restrict__ csr_buf, const double* __restrict__ dNx_csr,
                                                         const double* __restrict__ P, const double* __restrict__ P_csr,
                                                         const double* __restrict__ momentum,
                                                         const double* __restrict__ rhs_rest, double* __restrict__ out) {
    PN_SIM_PRIO();
    constexpr int NS = PN_GATHER_SLOTS;
    __shared__ double red[NS][30][3];
    const int k = blockIdx.x;
    const int t = threadIdx.x;
    const int slot = t / 30, q = t - slot * 30, c = q / 10;
    const int bg = csr_bg[k], cnt = csr_cnt[k];
    if (t < NS * 30) {
        double a0 = 0.0, a1 = 0.0, a2 = 0.0;
        const double* __restrict__ g = dNx_csr + (size_t)bg * 30 + q;
        int e = slot;
        if (P_csr) {  // every load is independent of every other
            const double* __restrict__ pc = P_csr + (size_t)bg * 9 + c;
            for (; e + 3 * NS < cnt; e += 4 * NS) {  // four entries in flight
                double gv[4], p0[4], p1[4], p2[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const size_t ee = (size_t)(e + NS * u);
                    gv[u] = g[ee * 30];
                    p0[u] = pc[ee * 9]; p1[u] = pc[ee * 9 + 3]; p2[u] = pc[ee * 9 + 6];
                }
#pragma unroll
                for (int u = 0; u < 4; u++) { a0 += p0[u] * gv[u]; a1 += p1[u] * gv[u]; a2 += p2[u] * gv[u]; }
            }
            for (; e < cnt; e += NS) {
                const double gv = g[(size_t)e * 30];
                a0 += pc[(size_t)e * 9] * gv;
                a1 += pc[(size_t)e * 9 + 3] * gv;
                a2 += pc[(size_t)e * 9 + 6] * gv;
            }
        } else {
            for (; e < cnt; e += NS) {
                const int v = csr_buf[bg + e] >> 3;
                const double gv = g[(size_t)e * 30];
                const double* __restrict__ Pv = P + (size_t)v * 9 + c;
                a0 += Pv[0] * gv;
                a1 += Pv[3] * gv;
                a2 += Pv[6] * gv;
            }
        }
        red[slot][q][0] = a0; red[slot][q][1] = a1; red[slot][q][2] = a2;
    }
    __syncthreads();
    if (t < 30) {
        const int x = t / 3, r = t - x * 3;  // output row x*3 + r of kernel k
        double s = 0.0;
        for (int sl = 0; sl < NS; sl++)
#pragma unroll
            for (int cc = 0; cc < 3; cc++) s += red[sl][cc * 10 + x][r];
        const size_t o = (size_t)k * 30 + t;
        out[o] = momentum[o] + s - rhs_rest[o];
    }
}

// Balanced form of the gather used by the step driver.  One workgroup per kernel leaves the launch as long as its longest list (chair:
// 770 entries against a mean of 206, and only 139 of 256 CUs busy), so the lists are cut into chunks of PN_GCH entries, one
// workgroup per chunk, each writing its 30 partial sums; the chunk sums of a kernel are added in ascending chunk order by the
// workgroup that completes its kernel's set (k_rhs_gather_chunk), so the result is still reproducible bit for bit.
// k_gather_plan (once per simulator, one workgroup) lays the chunks out: kc_bg[k] = first chunk of kernel k, chunk[b] = (first entry, count, kernel,
// chunks of that kernel); every kernel gets at least one chunk (an empty one if it has no entries), unused grid slots have kernel -1.
#ifndef PN_GCH
#define PN_GCH 64   // entries per chunk; the chunk kernel runs PN_GCH / 4 slots x 30 threads.  64 (512-thread workgroups) since round 4: 6.9 instead of 7.7 us alone, and beside the render
                    // lanes a launch of smaller workgroups finds room sooner (start-to-next-start 10.8 instead of 14.4 us; 32: 11.6; profiles/r04_sim_stamps.txt)
#endif
__global__ void __launch_bounds__(512) k_gather_plan(int n_k, int chunks_max, const int* __restrict__ csr_bg, const int* __restrict__ csr_cnt,
                                                     int* __restrict__ kc_bg, int4* __restrict__ chunk, int* __restrict__ kcount) {
    // exclusive scan of the kernels' chunk counts by the whole workgroup (one lane walking the n_k kernels took 40 us of every substep)
    __shared__ int wsum[8];
    __shared__ int carry_s;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (int base = 0; base < n_k; base += 512) {
        const int k = base + (int)threadIdx.x;
        const int cnt = k < n_k ? csr_cnt[k] : 0;
        const int nc = k < n_k ? max((cnt + PN_GCH - 1) / PN_GCH, 1) : 0;
        int inc = nc;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_up(inc, o);
            if (lane >= o) inc += u;
        }
        if (lane == 63) wsum[wid] = inc;
        __syncthreads();
        int woff = 0, total = 0;
        for (int w = 0; w < 8; w++) { woff += (w < wid) ? wsum[w] : 0; total += wsum[w]; }
        const int first_chunk = carry_s + woff + inc - nc;
        if (k < n_k) {
            kc_bg[k] = first_chunk;
            const int bg = csr_bg[k];
            for (int j = 0; j < nc; j++)  // one load tells a workgroup its work
                chunk[first_chunk + j] = make_int4(bg + j * PN_GCH, max(min(PN_GCH, cnt - j * PN_GCH), 0), k, nc);
            kcount[k] = 0;
        }
        __syncthreads();
        if (threadIdx.x == 0) carry_s += total;
        __syncthreads();
    }
    const int n_chunks = carry_s;
    if (threadIdx.x == 0) kc_bg[n_k] = n_chunks;
    for (int b = n_chunks + threadIdx.x; b < chunks_max; b += blockDim.x) chunk[b] = make_int4(0, 0, -1, 0);  // unused tail of the grid
}

// The workgroup that completes its kernel's set of chunks ("last arriver") also adds them up, in ascending chunk order, and writes
// momentum + sum - rhs_rest: the sums need no launch of their own.  The XCDs' L2s are not coherent with each
// other, so the chunk sums go out as agent-scope stores (written through to the memory side), a workgroup waits for their acknowledgement before it bumps
// its kernel's arrival counter (agent-scope atomic at the memory side), and the last arriver — the one that counts `chunks` arrivals — reads all sums
// with agent-scope loads and stores 0 back into the counter: nobody else arrives at it before the next launch, so the counter is cyclic and a simulator
// that runs for days never wraps it (rounds 1-3 let it grow and tested (n % chunks) == 0, which loses its phase at 2^31 for chunk counts that do not divide 2^32).
__global__ void __launch_bounds__(PN_GCH * 8) k_rhs_gather_chunk(const int4* __restrict__ chunk, const double* __restrict__ dNx_csr,
                                                                  const double* __restrict__ P_csr, double* part, int* kcount,
                                                                  const int* __restrict__ kc_bg, const double* __restrict__ momentum,
                                                                  const double* __restrict__ rhs_rest, double* __restrict__ tot) {
    PN_SIM_STAMP(2);
    PN_SIM_PRIO();
    constexpr int NS = PN_GCH / 4;
    __shared__ double red[NS][30][3];
    __shared__ int last_s;
    const int b = blockIdx.x;
    const int4 ch = chunk[b];
    const int bg = ch.x, cnt = ch.y, kern = ch.z, nck = ch.w;
    if (kern < 0) return;  // the grid is the host-side upper bound 8 n_IP / PN_GCH + n_k
    const int t = threadIdx.x;
    const int slot = t / 30, q = t - slot * 30, c = q / 10;
    if (t < NS * 30) {
        double a0 = 0.0, a1 = 0.0, a2 = 0.0;
        const double* __restrict__ g = dNx_csr + (size_t)bg * 30 + q;
        const double* __restrict__ pc = P_csr + (size_t)bg * 9 + c;
        double gv[4], p0[4], p1[4], p2[4];  // PN_GCH / NS = 4 entries per slot, all loads independent
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int e = slot + NS * u;
            const bool on = e < cnt;
            const size_t ee = on ? (size_t)e : 0;
            gv[u] = on ? g[ee * 30] : 0.0;
            p0[u] = on ? pc[ee * 9] : 0.0; p1[u] = on ? pc[ee * 9 + 3] : 0.0; p2[u] = on ? pc[ee * 9 + 6] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 4; u++) { a0 += p0[u] * gv[u]; a1 += p1[u] * gv[u]; a2 += p2[u] * gv[u]; }
        red[slot][q][0] = a0; red[slot][q][1] = a1; red[slot][q][2] = a2;
    }
    __syncthreads();
    // 30 outputs x NS slots: NS consecutive lanes add slot sl of output o (its three columns), then a fixed xor tree over those lanes
    // (30 threads adding 96 values each one after the other were 2.5 us of this kernel's 6.3)
    static_assert(NS == 32 || NS == 16 || NS == 8, "a power-of-two group of lanes per output");
    if (t < 30 * NS) {
        const int o = t / NS, sl = t % NS;
        const int x = o / 3, r = o - x * 3;
        double s = (red[sl][x][r] + red[sl][10 + x][r]) + red[sl][20 + x][r];
#pragma unroll
        for (int m = NS / 2; m > 0; m >>= 1) s += shfl_xor_d(s, m);
        if (sl == 0) __hip_atomic_store(part + (size_t)b * 30 + o, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __builtin_amdgcn_s_waitcnt(0);  // the sums are at the memory side
    __syncthreads();
    if (t == 0) {
        const int old = __hip_atomic_fetch_add(kcount + kern, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last_s = (old + 1) == nck;
        if (last_s) __hip_atomic_store(kcount + kern, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-armed for the next launch
    }
    __syncthreads();
    if (!last_s || t >= 30) return;
    const int b0 = kc_bg[kern];
    double sum = 0.0;
    for (int j0 = 0; j0 < nck; j0 += 8) {  // ascending chunk order, eight loads in flight (unconditional, clamped)
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = __hip_atomic_load(part + (size_t)(b0 + min(j0 + u, nck - 1)) * 30 + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int u = 0; u < 8; u++) if (j0 + u < nck) sum += v[u];
    }
    const size_t o = (size_t)kern * 30 + t;
    tot[o] = momentum[o] + sum - rhs_rest[o];
}

extern "C" int pn_sim_collect_rhs(int n_k, double dx, const int* csr_bg, const int* csr_cnt, const int* csr_buf, const double* mu, const double* lam,
                                  const double* dNx, const double* RF, const double* VF, double* rhs, void* stream) {
    PN_REQUIRE(n_k > 0 && csr_bg && csr_cnt && csr_buf && mu && lam && dNx && RF && VF && rhs);
    k_rhs_gather<<<pn_div_up(n_k, 4), 256, 0, (hipStream_t)stream>>>(n_k, pow(dx, 3.0), csr_bg, csr_cnt, csr_buf, mu, lam, dNx, RF, VF, nullptr, nullptr,
                                                                   nullptr, rhs);
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

// ------------------------------------------------------------------------------------------------ stepforward
__global__ void __launch_bounds__(256) k_step_begin(int n3, double dt, const double* __restrict__ dof, const double* __restrict__ vel,
                                                    double* __restrict__ tilde, double* __restrict__ last, int* __restrict__ coop_ctl = nullptr) {
    PN_SIM_PRIO();
    const int i = threadIdx.x + blockIdx.x * blockDim.x;
    // persistent form: the barrier counters of k_substep_coop start every substep at zero (the previous substep's launch has ended: stream order)
    if (coop_ctl && blockIdx.x == 0 && threadIdx.x < 10) coop_ctl[threadIdx.x * 32] = 0;  // PnCoopCtl: xcd_ctr[8], glob, gen
    if (i >= n3) return;
    const double d = dof[i];
    tilde[i] = d + dt * vel[i];  // solver.py:575
    last[i] = d;                 // dof_last = dof.clone() (:597)
}
__global__ void __launch_bounds__(256) k_step_end(int n3, double dt, const double* __restrict__ dof, const double* __restrict__ last,
                                                  double* __restrict__ vel) {
    PN_SIM_PRIO();
    const int i = threadIdx.x + blockIdx.x * blockDim.x;
    if (i >= n3) return;
    vel[i] = (dof[i] - last[i]) / dt * 0.998;  // solver.py:602
}

static inline uint64_t pn_gather_chunks_max(int n_k, int n_IP) { return (uint64_t)n_IP * 8 / PN_GCH + (uint64_t)n_k; }
// tilde, last, momentum, tot [n_k*30 each] | P [n_IP*9] | P_csr [n_IP*8*9] | chunk sums [chunks_max*30] | plan: kc_bg [n_k+1] ints, kcount [n_k] ints,
// chunk [chunks_max] int4 | Vstore [n_IP*9]
extern "C" uint64_t pn_sim_work_doubles(int n_k, int n_IP) {
    const uint64_t ch = pn_gather_chunks_max(n_k, n_IP);
    return (uint64_t)n_k * 30 * 4 + (uint64_t)n_IP * 9 + (uint64_t)n_IP * 8 * 9 + ch * 30 + 2 * (((uint64_t)n_k + 2) / 2 + 1) + 2 * ch + 2 + (uint64_t)n_IP * 9;
}
// the plan's three arrays behind the chunk sums
struct PnGatherPlan { int* kc_bg; int* kcount; int4* chunk; };
static inline PnGatherPlan pn_gather_plan_ptrs(double* part, uint64_t chunks_max, int n_k) {
    PnGatherPlan p;
    const size_t slot = ((size_t)n_k + 2) & ~(size_t)1;  // ints, even: every array starts on 8 bytes; the chunk table on 16
    p.kc_bg = reinterpret_cast<int*>(part + chunks_max * 30);
    p.kcount = p.kc_bg + slot;
    p.chunk = reinterpret_cast<int4*>((reinterpret_cast<uintptr_t>(p.kcount + slot) + 15) & ~(uintptr_t)15);
    return p;
}
// where the per-IP rotations of the warm-started SVD live in `work` (behind everything else)
static inline double* pn_sim_vstore(double* work, int n_k, int n_IP) { return work + (pn_sim_work_doubles(n_k, n_IP) - (uint64_t)n_IP * 9); }

__global__ void __launch_bounds__(256) k_vstore_identity(int n_IP, double* __restrict__ Vstore) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n_IP * 9) Vstore[t] = (t % 9) % 4 == 0 ? 1.0 : 0.0;
}

// Once per simulator (and again whenever `work` is re-allocated): what a substep needs in `work` but does not depend on the state — the chunk
// layout of the balanced gather (rounds 1-2 rebuilt it in every substep: one launch of the ~42) and identity rotations for the warm-started SVD.
extern "C" int pn_sim_prepare(int n_k, int n_IP, const int* csr_bg, const int* csr_cnt, double* work, void* stream) {
    PN_REQUIRE(n_k > 0 && n_IP > 0 && csr_bg && csr_cnt && work);
    hipStream_t st = (hipStream_t)stream;
    const int n3 = n_k * 30;
    const uint64_t chunks_max = pn_gather_chunks_max(n_k, n_IP);
    double* part = work + 4 * (size_t)n3 + (size_t)n_IP * 9 + (size_t)n_IP * 8 * 9;
    const PnGatherPlan gp = pn_gather_plan_ptrs(part, chunks_max, n_k);
    k_gather_plan<<<1, 512, 0, st>>>(n_k, (int)chunks_max, csr_bg, csr_cnt, gp.kc_bg, gp.chunk, gp.kcount);
    k_vstore_identity<<<pn_div_up((uint64_t)n_IP * 9, 256), 256, 0, st>>>(n_IP, pn_sim_vstore(work, n_k, n_IP));
    PN_LAUNCH_CHECK();
    return PN_OK;
}

extern "C" int pn_sim_stepforward(int n_k, int n_IP, int iters, double dt, double dx, const int* topo, const int* csr_bg, const int* csr_cnt,
                                  const int* csr_buf, const double* mu, const double* lam, const double* dNx, const double* dNx_csr,
                                  const int* csr_pos, const double* Ainv, const double* Mmat, const double* dof_rest, const double* rhs_rest,
                                  const double* rhs_gravity, const double* dof_f, double* dof, double* dof_vel, double* work, int prepared, int mcadams_sweeps,
                                  void* stream) {
    PN_REQUIRE(n_k > 0 && n_IP > 0 && iters >= 0 && topo && csr_bg && csr_cnt && csr_buf && mu && lam && dNx && Ainv && Mmat);
    PN_REQUIRE(dof_rest && rhs_rest && rhs_gravity && dof_f && dof && dof_vel && work && pn_svd_sweeps_ok(mcadams_sweeps));
    hipStream_t st = (hipStream_t)stream;
    const int n = n_k * 10, n3 = n * 3;
    double* tilde = work;
    double* last = work + n3;
    double* momentum = work + 2 * (size_t)n3;
    double* tot = work + 3 * (size_t)n3;
    double* P = work + 4 * (size_t)n3;
    double* P_csr = P + (size_t)n_IP * 9;
    const uint64_t chunks_max = pn_gather_chunks_max(n_k, n_IP);
    double* part = P_csr + (size_t)n_IP * 8 * 9;
    const PnGatherPlan gp = pn_gather_plan_ptrs(part, chunks_max, n_k);
    int* kc_bg = gp.kc_bg;
    int4* chunk = gp.chunk;
    const double dx3 = pow(dx, 3.0);
    const bool pcsr = dNx_csr && csr_pos;
    // balanced gather: the lists cut into chunks of PN_GCH entries, the chunk kernel's last arriver sums them.  Without the CSR-ordered copies, or for a
    // right-hand side above ~159 KB, one gather workgroup per kernel instead (k_rhs_gather_csr / k_rhs_gather)
    const bool chunked = pcsr && (size_t)n3 * sizeof(double) <= 160 * 1024 - 1024;
    if (chunked && !prepared) k_gather_plan<<<1, 512, 0, st>>>(n_k, (int)chunks_max, csr_bg, csr_cnt, kc_bg, chunk, gp.kcount);
    double* Vstore = prepared ? pn_sim_vstore(work, n_k, n_IP) : nullptr;   // warm-started SVD (prepared == 0: every SVD starts from the identity)
    // k_elastic in one-wave workgroups: a lane's 60 loads (its kernel's 30 DOFs, its 30 shape-function gradients) are 240-B blocks of its own, so every
    // load instruction touches 64 cache lines and keeps the CU's address path busy for ~140 cycles; with 256-thread workgroups the 447 waves of the
    // chair sat four to a CU on 112 of the 256 CUs and queued on that path (31.9 -> 28.3 us per local/global iteration; 16-byte loads on top: nothing)
    const uint32_t el_blocks = pn_div_up((uint64_t)n_IP * 8, 64);
    // ... and the matrix products in one-wave workgroups (two rows each) as well: beside the render lanes' persistent workgroups a launch starts when its
    // workgroups find room, and a single wave finds it sooner than four (start-to-start gap behind k_matvec3 in the pipeline: profiles/r04_sim_stamps.txt)
    const uint32_t mv_blocks = pn_div_up(n, 2);
    // the substep's two elementwise launches ride on the matrix products next to them; k_step_begin / k_step_end as launches when the gather is not
    // chunked or there is no iteration to carry the epilogue
    const bool ends = chunked && iters >= 1;
    if (ends) {
        k_matvec3<<<mv_blocks, 64, 0, st>>>(n, Mmat, dof, momentum, 1, dof_f, rhs_gravity, dof_vel, dt, last);  // dof_tilde on the fly, dof_last = dof
    } else {
        k_step_begin<<<pn_div_up(n3, 256), 256, 0, st>>>(n3, dt, dof, dof_vel, tilde, last);
        k_matvec3<<<mv_blocks, 64, 0, st>>>(n, Mmat, tilde, momentum, 1, dof_f, rhs_gravity);  // compute_momentum (:574-576)
    }
    for (int it = 0; it < iters; it++) {
        if (mcadams_sweeps)
            k_elastic<true><<<el_blocks, 64, 0, st>>>(n_IP, topo, dNx, dof, nullptr, nullptr, nullptr, pcsr ? nullptr : P, mu, lam, dx3, pcsr ? csr_pos : nullptr,
                                                      pcsr ? P_csr : nullptr, Vstore, mcadams_sweeps);
        else
            k_elastic<false><<<el_blocks, 64, 0, st>>>(n_IP, topo, dNx, dof, nullptr, nullptr, nullptr, pcsr ? nullptr : P, mu, lam, dx3, pcsr ? csr_pos : nullptr,
                                                       pcsr ? P_csr : nullptr, Vstore);
        if (chunked)
            k_rhs_gather_chunk<<<(uint32_t)chunks_max, PN_GCH * 8, 0, st>>>(chunk, dNx_csr, P_csr, part, gp.kcount, kc_bg, momentum, rhs_rest, tot);
        else if (dNx_csr)  // CSR-ordered copy of dNx available: the coalesced one-workgroup-per-kernel gather
            k_rhs_gather_csr<<<n_k, 1024, 0, st>>>(n_k, csr_bg, csr_cnt, csr_buf, dNx_csr, P, pcsr ? P_csr : nullptr, momentum, rhs_rest, tot);
        else
            k_rhs_gather<<<pn_div_up(n_k, 4), 256, 0, st>>>(n_k, dx3, csr_bg, csr_cnt, csr_buf, mu, lam, dNx, nullptr, nullptr, P, momentum, rhs_rest, tot);
        if (ends && it == iters - 1) k_matvec3<<<mv_blocks, 64, 0, st>>>(n, Ainv, tot, dof, 3, dof_rest, last, nullptr, dt, nullptr, dof_vel);  // + vel (:602)
        else k_matvec3<<<mv_blocks, 64, 0, st>>>(n, Ainv, tot, dof, 2, dof_rest, nullptr);  // x = G @ rhs ; dof = dof_rest + x (:600-601)
    }
    if (!ends) k_step_end<<<pn_div_up(n3, 256), 256, 0, st>>>(n3, dt, dof, last, dof_vel);
    PN_LAUNCH_CHECK();
    return PN_OK;
}

// ------------------------------------------------------------------------------------------------ the substep in its CELL form (round 5)
// calc_elastic and collect_rhs_IP of one local/global iteration as ONE launch (k_cells_elastic_gather), the dense product as the other: 21 launches per
// substep instead of 31.  What a launch of this chain costs is its boundary (~4.5 us of the 6.8-9.2 us from one start to the next, alone; beside the render
// lanes every launch also waits for room on a CU), so the way to a shorter substep is fewer of them.
// The reference's topology makes the merge cheap: an integration point's 8 neighbour kernels are the corners of the KERNEL-GRID CELL it lies in
// (solver.py:186-205), so all points of one cell share the same 8 kernels, slot i meaning the same kernel for each of them.  The host sorts the points by
// cell and cuts every cell into chunks of <= PN_CELL_IPS points (simulator/solver.py: _build_cells); a workgroup takes one chunk:
//   * 8 lanes per point as in k_elastic, but the chunk's shape-function gradients come from a copy laid out for it ([chunk][wave][15][64 lanes] double2:
//     every load instruction reads 1 KB contiguous, k_elastic's touched 64 cache lines) and the 8 lanes of a point read the 8 kernels' DOFs that the whole
//     workgroup shares (8 distinct 240-B rows per instruction instead of 64);
//   * the point's stress times ITS OWN gradients — still in the lane's registers from the deformation gradient — is its contribution to its 8 kernels:
//     no P_csr, no dNx_csr, no index;
//   * summed over the chunk's points in LDS in a fixed order (point after point) into 8 x 30 partial sums, stored write-through; the workgroup that
//     completes a kernel's set of partial sums (cyclic arrival counters, as k_rhs_gather_chunk; the sums of a kernel lie side by side, kp_pos) adds them
//     by a fixed tree and writes momentum + sum - rhs_rest.  Bit-reproducible run to run; against the CSR form the summation order differs (1e-16 relative).
#ifndef PN_CELL_WAVES
#define PN_CELL_WAVES 4
#endif
#define PN_CELL_IPS (PN_CELL_WAVES * 8)
static_assert(PN_CELL_WAVES == 4, "k_cells_elastic_gather's t < 240 phases and its LDS reduction assume 256-thread workgroups");
#ifndef PN_CELL_SVD_PACK
#define PN_CELL_SVD_PACK 1
#endif
#ifndef PN_CELL_SVD_TOL
#define PN_CELL_SVD_TOL 1e-22
#endif
#ifndef PN_CELL_SVD_SKIP
#define PN_CELL_SVD_SKIP 1e-23
#endif
#define PN_CELL_TAB_INTS 12   // per chunk: {points, kernel of slot 0..7, 0, 0, 0}
#define PN_CELL_RSTRIDE 66    // doubles per output row of the LDS reduction buffer (64 lanes + 2: rows 4 banks apart)

template <bool MC>
__global__ void __launch_bounds__(PN_CELL_WAVES * 64) k_cells_elastic_gather(const int* __restrict__ chunk_tab, const double2* __restrict__ dNx_cell,
                                                                              const double* __restrict__ mu_cell, const double* __restrict__ lam_cell,
                                                                              const double* __restrict__ dof, double dx3, double* __restrict__ Vstore,
                                                                              double* part, int* kcount, const int* __restrict__ kp_bg,
                                                                              const int* __restrict__ kp_pos, const double* __restrict__ momentum,
                                                                              const double* __restrict__ rhs_rest, double* __restrict__ tot, int mc_sweeps) {
    PN_SIM_STAMP(1);
    PN_SIM_PHASE_DECL;
    PN_SIM_PHASE(10);
    PN_SIM_PRIO();
    constexpr int NW = PN_CELL_WAVES, B = PN_CELL_IPS;
    __shared__ double red[NW][30][PN_CELL_RSTRIDE];
    __shared__ int s_last[8], s_k[8], s_b0[8], s_n[8];
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6, i = lane & 7;
    const int vl = w * 8 + (lane >> 3);                       // the point's place in the chunk
    const int* __restrict__ tab = chunk_tab + (size_t)b * PN_CELL_TAB_INTS;
    const int count = tab[0];
    const int kid = tab[1 + i];
    const bool live = vl < count;
    const int my_pos = t < 240 ? kp_pos[b * 8 + (t & 7)] : 0; // where this thread's partial sum goes (asked for now, needed at the end)
    if (t < 8) {                                              // the 8 kernels' runs of partial sums, for whoever completes them (read behind two barriers)
        const int k = tab[1 + t];
        const int b0 = kp_bg[k];
        s_k[t] = k; s_b0[t] = b0; s_n[t] = kp_bg[k + 1] - b0;
    }
    const size_t vg = (size_t)b * B + vl;                     // ... and in the chunk-ordered per-point arrays
    // Who decomposes.  PN_CELL_SVD_PACK: lane l < PN_CELL_IPS of wave 0 takes point l of the chunk — ONE wave issues the SVD's ~900 dependent instructions
    // for all 32 points instead of four waves issuing them for 8 lanes each (the chain is as long either way, but beside the render lanes what the substep
    // costs is vector issue: the lane-sparse form was 3.4 M of the frame's ~107 M vector instructions, in fp64).  F goes there and P comes back through LDS.
    // Otherwise: lane 0 of the point's own 8-lane group.
#if PN_CELL_SVD_PACK
    const bool svd_lane = w == 0 && lane < B && lane < count;
    const size_t vs = (size_t)b * B + (size_t)(lane & (B - 1));
#else
    const bool svd_lane = i == 0 && live;
    const size_t vs = vg;
#endif
    // the previous iteration's rotation, asked for before anything else: it is needed last
    M3 Q0;
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) Q0.m[r][c] = svd_lane ? Vstore[vs * 9 + r * 3 + c] : 0.0;
    const double m_ = svd_lane ? mu_cell[vs] : 0.0, l_ = svd_lane ? lam_cell[vs] : 0.0;
    double g[30], d[30];                                      // g[c * 10 + x] = dNx[v, i, c, x] (zeros behind the chunk's last point); d[x * 3 + r]
    {
        const double2* __restrict__ g2 = dNx_cell + ((size_t)b * NW + w) * 15 * 64 + lane;
        const double2* __restrict__ d2 = reinterpret_cast<const double2*>(dof + (size_t)kid * 30);
#pragma unroll
        for (int j = 0; j < 15; j++) {
            const double2 gv = g2[j * 64], dv = d2[j];
            g[2 * j] = gv.x; g[2 * j + 1] = gv.y;
            d[2 * j] = dv.x; d[2 * j + 1] = dv.y;
        }
    }
    M3 Fm;
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) Fm.m[r][c] = 0.0;
#pragma unroll
    for (int x = 0; x < 10; x++)                              // the same sums in the same order as k_elastic
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const double gg = g[c * 10 + x];
            Fm.m[0][c] += d[x * 3] * gg;
            Fm.m[1][c] += d[x * 3 + 1] * gg;
            Fm.m[2][c] += d[x * 3 + 2] * gg;
        }
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            double s = Fm.m[r][c];
            s += shfl_xor_d(s, 1);
            s += shfl_xor_d(s, 2);
            s += shfl_xor_d(s, 4);
            Fm.m[r][c] = s;
        }
    PN_SIM_PHASE(11);
    double Pm[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#if PN_CELL_SVD_PACK
    __shared__ double s_F[PN_CELL_IPS][9], s_P[PN_CELL_IPS][9];
    if (i == 0) {
#pragma unroll
        for (int q = 0; q < 9; q++) s_F[vl][q] = Fm.m[q / 3][q % 3];
    }
    __syncthreads();
    if (svd_lane) {
#pragma unroll
        for (int q = 0; q < 9; q++) Fm.m[q / 3][q % 3] = s_F[lane][q];
    }
#endif
    if (svd_lane) {
        M3 U, V;
        double sig[3], sp[3];
        // off-diagonals below 1e-11 of the diagonal (1e-22 on the squares; pairs below 3e-12 are not rotated): seven digits beyond the 1e-4 relative bar
        // of the DOF displacements; against 1e-24 the third sweep — two take a warm-started decomposition from 1e-3 to 1e-12 — is mostly not run
        if (MC) {
            svd3_mcadams(Fm, U, sig, V, mc_sweeps);   // PN_SIM_SVD=mcadams: the published algorithm, fixed sweeps, no warm start (Vstore untouched)
        } else {
            svd3(Fm, U, sig, V, &Q0, PN_CELL_SVD_TOL, PN_CELL_SVD_SKIP);
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int c = 0; c < 3; c++) Vstore[vs * 9 + r * 3 + c] = V.m[r][c];
        }
        volume_invariant_project(sig, sp);
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const double R = U.m[r][0] * V.m[c][0] + U.m[r][1] * V.m[c][1] + U.m[r][2] * V.m[c][2];
                const double Vv = U.m[r][0] * sp[0] * V.m[c][0] + U.m[r][1] * sp[1] * V.m[c][1] + U.m[r][2] * sp[2] * V.m[c][2];
                Pm[r * 3 + c] = dx3 * (m_ * R + l_ * Vv);
            }
    }
    PN_SIM_PHASE(12);
#if PN_CELL_SVD_PACK
    if (w == 0 && lane < B) {
#pragma unroll
        for (int q = 0; q < 9; q++) s_P[lane][q] = Pm[q];   // (zeros behind the chunk's last point)
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 9; q++) Pm[q] = s_P[vl][q];
#else
    {
        const int src = lane & ~7;
#pragma unroll
        for (int q = 0; q < 9; q++) {
            int2 tt = *reinterpret_cast<int2*>(&Pm[q]);
            tt.x = __shfl(tt.x, src);
            tt.y = __shfl(tt.y, src);
            Pm[q] = *reinterpret_cast<double*>(&tt);
        }
    }
#endif
    // this (point, slot)'s contribution to its kernel: out[x][r] = sum_c P[r][c] dNx[c][x] (cuda_utils.py:124-151), row x * 3 + r of the wave's buffer
#pragma unroll
    for (int x = 0; x < 10; x++)
#pragma unroll
        for (int r = 0; r < 3; r++)
            red[w][x * 3 + r][lane] = (Pm[r * 3] * g[x] + Pm[r * 3 + 1] * g[10 + x]) + Pm[r * 3 + 2] * g[20 + x];
    __syncthreads();
    PN_SIM_PHASE(13);
    // 240 outputs (slot, row): the chunk's points one after the other, waves in ascending order
    if (t < 240) {
        const int o = t >> 3, sl = t & 7;
        double s = 0.0;
#pragma unroll
        for (int ww = 0; ww < NW; ww++)
#pragma unroll
            for (int p = 0; p < 8; p++) s += red[ww][o][p * 8 + sl];
        __hip_atomic_store(part + (size_t)my_pos * 30 + o, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // its place in its kernel's run
    }
    __builtin_amdgcn_s_waitcnt(0);  // the sums are at the memory side
    __syncthreads();
    PN_SIM_PHASE(14);
    if (t < 8) {
        const int k = s_k[t];
        const int old = __hip_atomic_fetch_add(kcount + k, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = (old + 1) == s_n[t];
        if (last) __hip_atomic_store(kcount + k, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-armed for the next launch
        s_last[t] = last;
    }
    __syncthreads();
    PN_SIM_PHASE(15);
    // The kernels this workgroup completed: none for most, but the workgroups that arrive last complete several — the very last one all 8 of its own —
    // and the launch ends with them: one thread per (completed kernel, output row), all at once; a row's partial sums lie 240 B apart in the kernel's run
    // (kp_pos) and are added in ascending order, sixteen loads in flight.
    if (t < 240) {
        const int sl = t / 30, q = t - sl * 30;
        if (s_last[sl]) {
            const int k = s_k[sl], b0 = s_b0[sl], n = s_n[sl];
            const size_t o = (size_t)k * 30 + q;
            const double m0 = momentum[o], r0 = rhs_rest[o];
            const double* __restrict__ src = part + (size_t)b0 * 30 + q;
            double sum = 0.0;
            for (int j0 = 0; j0 < n; j0 += 16) {   // (32 at a time measured slower: 0.215 against 0.208 ms per substep)
                double v[16];
#pragma unroll
                for (int u = 0; u < 16; u++) v[u] = __hip_atomic_load(src + (size_t)min(j0 + u, n - 1) * 30, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
                for (int u = 0; u < 16; u++) if (j0 + u < n) sum += v[u];
            }
            tot[o] = m0 + sum - r0;
        }
    }
    PN_SIM_PHASE(16);
    PN_SIM_PHASE_FLUSH;
}

extern "C" int pn_sim_cells_chunk_ips(void) { return PN_CELL_IPS; }
// last, momentum, tot [30 n_k each] | partial sums [n_chunks * 240] | rotations [n_chunks * PN_CELL_IPS * 9] | arrival counters [n_k ints]
extern "C" uint64_t pn_sim_cells_work_doubles(int n_k, int n_chunks) {
    return (uint64_t)n_k * 30 * 3 + (uint64_t)n_chunks * 240 + (uint64_t)n_chunks * PN_CELL_IPS * 9 + ((uint64_t)n_k + 2) / 2;
}
__global__ void __launch_bounds__(256) k_cells_prepare(int n_rot9, int n_k, double* __restrict__ Vstore, int* __restrict__ kcount) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n_rot9) Vstore[t] = (t % 9) % 4 == 0 ? 1.0 : 0.0;
    if (t < n_k) kcount[t] = 0;
}
extern "C" int pn_sim_cells_prepare(int n_k, int n_chunks, double* work, void* stream) {
    PN_REQUIRE(n_k > 0 && n_chunks > 0 && work);
    double* Vstore = work + (size_t)n_k * 90 + (size_t)n_chunks * 240;
    int* kcount = reinterpret_cast<int*>(Vstore + (size_t)n_chunks * PN_CELL_IPS * 9);
    const int n9 = n_chunks * PN_CELL_IPS * 9;
    k_cells_prepare<<<pn_div_up((uint64_t)std::max(n9, n_k), 256), 256, 0, (hipStream_t)stream>>>(n9, n_k, Vstore, kcount);
    PN_LAUNCH_CHECK();
    return PN_OK;
}

extern "C" int pn_sim_stepforward_cells(int n_k, int n_chunks, int iters, double dt, double dx, const int* chunk_tab, const double* dNx_cell,
                                        const double* mu_cell, const double* lam_cell, const int* kp_bg, const int* kp_pos, const double* Ainv,
                                        const double* Mmat, const double* dof_rest, const double* rhs_rest, const double* rhs_gravity, const double* dof_f,
                                        double* dof, double* dof_vel, double* work, int mcadams_sweeps, void* stream) {
    PN_REQUIRE(n_k > 0 && n_chunks > 0 && iters >= 1 && chunk_tab && dNx_cell && mu_cell && lam_cell && kp_bg && kp_pos && Ainv && Mmat);
    PN_REQUIRE(dof_rest && rhs_rest && rhs_gravity && dof_f && dof && dof_vel && work && pn_svd_sweeps_ok(mcadams_sweeps));
    hipStream_t st = (hipStream_t)stream;
    const int n = n_k * 10, n3 = n * 3;
    double* last = work;
    double* momentum = work + (size_t)n3;
    double* tot = work + 2 * (size_t)n3;
    double* part = work + 3 * (size_t)n3;
    double* Vstore = part + (size_t)n_chunks * 240;
    int* kcount = reinterpret_cast<int*>(Vstore + (size_t)n_chunks * PN_CELL_IPS * 9);
    const double dx3 = pow(dx, 3.0);
    const uint32_t mv_blocks = pn_div_up(n, 2);   // one-wave workgroups of two rows, as in pn_sim_stepforward
    // compute_momentum with dof_tilde = dof + dt * vel on the fly and dof_last = dof (solver.py:574-576,597)
    k_matvec3<<<mv_blocks, 64, 0, st>>>(n, Mmat, dof, momentum, 1, dof_f, rhs_gravity, dof_vel, dt, last);
    for (int it = 0; it < iters; it++) {
        if (mcadams_sweeps)
            k_cells_elastic_gather<true><<<n_chunks, PN_CELL_WAVES * 64, 0, st>>>(chunk_tab, reinterpret_cast<const double2*>(dNx_cell), mu_cell, lam_cell, dof,
                                                                                   dx3, Vstore, part, kcount, kp_bg, kp_pos, momentum, rhs_rest, tot,
                                                                                   mcadams_sweeps);
        else
            k_cells_elastic_gather<false><<<n_chunks, PN_CELL_WAVES * 64, 0, st>>>(chunk_tab, reinterpret_cast<const double2*>(dNx_cell), mu_cell, lam_cell, dof,
                                                                                    dx3, Vstore, part, kcount, kp_bg, kp_pos, momentum, rhs_rest, tot, 0);
        if (it == iters - 1) k_matvec3<<<mv_blocks, 64, 0, st>>>(n, Ainv, tot, dof, 3, dof_rest, last, nullptr, dt, nullptr, dof_vel);  // + vel (:602)
        else k_matvec3<<<mv_blocks, 64, 0, st>>>(n, Ainv, tot, dof, 2, dof_rest, nullptr);                                                // :600-601
    }
    PN_LAUNCH_CHECK();
    return PN_OK;
}

// ------------------------------------------------------------------------------------------------ the local/global iterations as ONE persistent kernel
// pn_sim_stepforward's loop is four dependent launches per local/global iteration, each 4-13 us although it moves a few hundred KB: what a launch costs
// is its chain of dependent memory round trips (index -> data -> result), not its boundary.  k_substep_coop runs all `iters` iterations in ONE launch of
// n_wg workgroups (one per CU) that keep everything state-independent where a round trip is not needed:
//   * registers: this workgroup's rows of A^-1 (rpw rows x n columns over 512 threads), the dNx rows of its piece of a kernel's CSR list;
//   * LDS: the shape-function gradients of its own integration points, the assembled right-hand side, the staged stresses of its piece.
// What is left per iteration is three all-to-all exchanges through memory (integration points -> pieces: P; pieces -> rows: piece sums; rows ->
// integration points: the new DOFs).  The XCDs' L2s are not coherent with each other and a release/acquire pair at device scope costs 13 us
// (tools/calib_barrier.hip), so nothing is fenced: exchanged values are written and read with relaxed AGENT-scope atomics (sc1: written through to /
// read from the memory side), a producer waits for its stores' acknowledgement (s_waitcnt vmcnt(0)) before it arrives at a counting barrier (arrivals
// per XCD-sized group of workgroups on separate cache lines, a generation word everybody polls).  tools/calib_exchange.hip: 4.2 us per exchange at
// 256 workgroups.  Every summation order is fixed (pieces in ascending entry order, waves in ascending order): bit-reproducible like the launch form.
// A workgroup that waits longer than ~1 s for a generation raises ctl->err and leaves (every other one follows): a launch whose workgroups cannot all
// be resident (a CU-masked stream, a debugger) fails instead of hanging the GPU; the host checks the flag (pn_sim_coop_status).
#define PN_COOP_THREADS 512
#define PN_COOP_NS (PN_COOP_THREADS / 30)  // 17 slots x 30 threads in the piece gather
#define PN_COOP_EU 16                       // piece entries per slot, register-resident: pieces of <= 272 entries
#define PN_COOP_RPW 8                       // rows of A^-1 per workgroup
#define PN_COOP_CU 4                        // columns per thread and row: n <= 2048
#define PN_COOP_IPW 32                      // integration points per workgroup (8 lanes each)
#define PN_COOP_MAXP 4                      // pieces per kernel at most
#define PN_COOP_ITERS 32                    // local/global iterations per launch at most (one exchange buffer per iteration, see k_substep_coop)

struct PnCoopCtl {  // every word that is polled or counted on a cache line of its own
    int xcd_ctr[8 * 32];
    int glob[32];
    int gen[32];
    int err[32];
};
struct PnCoopPlan {
    int n_wg, n_pieces, eu, ipw, rpw, max_pieces_per_kernel;
    size_t off_pieces, off_kp, off_psum, off_dofx, bytes;  // byte offsets inside the coop buffer
    size_t lds_bytes;
};

// cnt_host == NULL: sizes only, for `eu_known` entries per slot (0: the worst case PN_COOP_EU)
static int pn_coop_plan(int n_k, int n_IP, int n_wg, const int* cnt_host, PnCoopPlan* pl, int eu_known = 0) {
    const int n = n_k * 10;
    pl->n_wg = n_wg;
    pl->ipw = (n_IP + n_wg - 1) / n_wg;
    pl->rpw = (n + n_wg - 1) / n_wg;
    pl->eu = 0; pl->n_pieces = 0; pl->max_pieces_per_kernel = 0;
    if (n_wg < 8 || n_wg > 256 || pl->ipw > PN_COOP_IPW || pl->rpw > PN_COOP_RPW || n > PN_COOP_THREADS * PN_COOP_CU) return 0;
    auto lds_for = [&](size_t eu_l) {
        const size_t xs = std::max((size_t)n * 3, eu_l * PN_COOP_NS * 9 + (size_t)PN_COOP_NS * 90);
        return ((size_t)pl->ipw * 240 + xs + (size_t)n * 3 + eu_l * PN_COOP_NS * 30 + (size_t)pl->ipw * 9) * sizeof(double) + (((size_t)n_k + 2) & ~(size_t)1) * sizeof(int);
    };
    if (cnt_host) {
        // the longest pieces up to 12 entries per slot (204 entries) that fit the LDS, where the piece's dNx rows live: fewer pieces, fewer kernels whose
        // list is cut.  (16 per slot fit the chair at 160 KB of LDS and measured slower: 0.265 against 0.241 ms per substep.)
        const int eu_cap = (int)std::min<uint32_t>(pn_env_u32("PN_SIM_COOP_EU", 12), PN_COOP_EU);
        for (int eu = eu_cap; eu >= 1 && !pl->eu; eu--) {
            if (lds_for(eu) > 160 * 1024) continue;
            const int pmax = eu * PN_COOP_NS;
            long np = 0; int mp = 0;
            for (int k = 0; k < n_k; k++) { const int c = (cnt_host[k] + pmax - 1) / pmax; np += c; mp = std::max(mp, c); }
            if (np <= n_wg && mp <= PN_COOP_MAXP) { pl->eu = eu; pl->n_pieces = (int)np; pl->max_pieces_per_kernel = mp; }
        }
        if (!pl->eu) return 0;
    }
    pl->off_pieces = sizeof(PnCoopCtl);
    pl->off_kp = pl->off_pieces + (size_t)n_wg * sizeof(int4);
    pl->off_psum = (pl->off_kp + (size_t)(n_k + 1) * sizeof(int) + 127) & ~(size_t)127;
    pl->off_dofx = pl->off_psum + (size_t)PN_COOP_ITERS * n_wg * 30 * sizeof(double);  // psum: one [n_wg][30] block per iteration
    pl->bytes = pl->off_dofx + (size_t)PN_COOP_ITERS * n * 3 * sizeof(double);            // dofx: one DOF vector per iteration
    // LDS: Ds [ipw*240] | Xs [n*3] (aliased by Ps [eu*NS*9]) | Gs [eu*NS*30] | Qs [ipw*9] | red [NS*90] | pk [n_wg ints]
    pl->lds_bytes = lds_for(cnt_host ? pl->eu : (eu_known ? eu_known : 1));  // without the lists: does the smallest piece size fit at all
    return pl->lds_bytes <= 160 * 1024;
}

__device__ __forceinline__ void st_agent(double* p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ double ld_agent(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// A value another workgroup wrote (st_agent: through to the memory side) into a location that NO wave has read before in this launch: the piece sums
// and the DOF vector are exchanged through one buffer per iteration, and every wave starts the kernel with an agent-scope acquire fence (this XCD's L2
// and the CU's L1 hold nothing stale from earlier launches).  Such a location cannot be in any cache before its writer's barrier, so an ordinary cached
// load is coherent — and the 256 workgroups that all read the same 51 KB of piece sums (and the same DOF blocks) fetch them from their XCD's L2 after
// the first one instead of 13 MB per iteration from the memory side with sc1 loads (assembly phase 3.1 -> us).  Relaxed atomic at workgroup scope: the
// compiler may neither cache nor hoist it.
__device__ __forceinline__ double ld_fresh(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// Cross-lane sums on the DPP path (VALU moves) instead of ds_bpermute: a shuffle of a double is two LDS-crossbar operations, and the 18 x 6 of them in
// the first version of the rows phase took 5 us of every iteration.
template <int CTRL>
__device__ __forceinline__ double dpp_d(double v) {
    int2 tt = *reinterpret_cast<int2*>(&v);
    tt.x = __builtin_amdgcn_update_dpp(0, tt.x, CTRL, 0xf, 0xf, false);
    tt.y = __builtin_amdgcn_update_dpp(0, tt.y, CTRL, 0xf, 0xf, false);
    return *reinterpret_cast<double*>(&tt);
}
__device__ __forceinline__ double wave_sum_d(double v) {  // every lane gets the sum; fixed tree
    v += dpp_d<0xB1>(v);   // quad_perm [1,0,3,2]
    v += dpp_d<0x4E>(v);   // quad_perm [2,3,0,1]
    v += dpp_d<0x141>(v);  // row_half_mirror
    v += dpp_d<0x140>(v);  // row_mirror
    v += shfl_xor_d(v, 16);
    v += shfl_xor_d(v, 32);
    return v;
}

// All workgroups have arrived at generation g (counted from the launch's base) and their earlier agent-scope stores are at the memory side.
__device__ __forceinline__ bool coop_sync(PnCoopCtl* ctl, int g, int per_xcd, int xcd) {
    __shared__ int ok_s;
    __builtin_amdgcn_s_waitcnt(0);  // this thread's exchange stores acknowledged
    __syncthreads();
    if (threadIdx.x == 0) {
        int ok = 1;
        const int a = __hip_atomic_fetch_add(ctl->xcd_ctr + xcd * 32, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (a == per_xcd * g - 1) {
            const int gg = __hip_atomic_fetch_add(ctl->glob, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (gg == 8 * g - 1) __hip_atomic_store(ctl->gen, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        int spins = 0;
        while (__hip_atomic_load(ctl->gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - g < 0) {
            __builtin_amdgcn_s_sleep(1);
            if ((++spins & 1023) == 0) {
                if (spins > (1 << 21) || __hip_atomic_load(ctl->err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) {
                    __hip_atomic_store(ctl->err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    ok = 0;
                    break;
                }
            }
        }
        ok_s = ok;
    }
    __syncthreads();
    return ok_s != 0;
}

// CW / EU / NO: columns of its row of A^-1 per lane, piece entries per slot (both register-resident: the budget is 256 registers per thread at two
// waves per SIMD and the SVD of the integration-point phase needs ~120 of them), right-hand-side entries per thread in the assembly (30 n_k / 512)
template <int CW, int EU, int NO>
__global__ void __launch_bounds__(PN_COOP_THREADS) k_substep_coop(int n_k, int n_IP, int iters, double dt, double dx3, const int* __restrict__ topo,
                                                                  const int* __restrict__ csr_pos, const double* __restrict__ mu,
                                                                  const double* __restrict__ lam, const double* __restrict__ dNx,
                                                                  const double* __restrict__ dNx_csr, const double* __restrict__ Ainv,
                                                                  const double* __restrict__ dof_rest, const double* __restrict__ rhs_rest,
                                                                  const double* __restrict__ momentum, const double* __restrict__ last, double* dof,
                                                                  double* __restrict__ dof_vel, double* P_csr, double* __restrict__ Vstore, PnCoopCtl* ctl,
                                                                  const int4* __restrict__ pieces, const int* __restrict__ kp_bg, double* psum_all,
                                                                  double* dofx_all,
                                                                  int n_pieces, int eu, int ipw, int rpw, int max_rank, int dbg) {
    PN_SIM_PRIO();
    extern __shared__ double coop_lds[];
    const int n = n_k * 10, n3 = n * 3;
    const int t = threadIdx.x, w = blockIdx.x, G = gridDim.x, lane = t & 63, wid = t >> 6;
    double* Ds = coop_lds;                                   // [ipw * 240]: shape-function gradients of the own integration points
    const size_t ps_len = (size_t)eu * PN_COOP_NS * 9;
    const size_t xs_len = max((size_t)n3, ps_len + PN_COOP_NS * 90);
    double* Xs = Ds + (size_t)ipw * 240;                     // [xs_len]: right-hand side (rows phase); in the pieces phase the staged stresses Ps ...
    double* red = Xs + ps_len;                               // ... and behind them the [NS * 90] partial sums of the slots
    double* Cs = Xs + xs_len;                                // [n3]: momentum - rhs_rest, the state-independent part of the right-hand side
    double* Gs = Cs + n3;                                    // [eu * NS * 30]: the dNx rows of this workgroup's piece
    double* Qs = Gs + (size_t)eu * PN_COOP_NS * 30;          // [ipw * 9]: warm-start rotations of the own integration points
    int* kp_s = reinterpret_cast<int*>(Qs + (size_t)ipw * 9);  // [n_k + 1]: first piece of every kernel
    const int xcd = w & 7, per_xcd = (G + 7 - xcd) / 8;
    int g = 0;  // generations of this launch (k_step_begin cleared the counters)
    const bool fresh = !(dbg & 8);  // PN_SIM_COOP_DBG & 8: sc1 loads for everything exchanged, no fence (timing experiment)
    if (fresh && wid == 0) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // see ld_fresh (one wave per workgroup; the others pass the barrier below after it)
    // PN_SIM_COOP_DBG & 4: workgroup 0 accumulates the wall-clock ticks (100 MHz) of the eight phases of an iteration in ctl->err[8..] (tools/time_sim.py)
    __shared__ unsigned long long clk_s[10];
    const bool clk_on = (dbg & 4) && w == 0 && t == 0;
    if (clk_on) { for (int i = 0; i < 10; i++) clk_s[i] = 0; clk_s[9] = wall_clock64(); }
#define PN_COOP_CLK(i) do { if (clk_on) { const unsigned long long now_ = wall_clock64(); clk_s[i] += now_ - clk_s[9]; clk_s[9] = now_; } } while (0)

    // ---- state-independent residents
    const int v0 = w * ipw, nown = max(min(ipw, n_IP - v0), 0);
    for (int e = t; e < nown * 240; e += PN_COOP_THREADS) Ds[e] = dNx[(size_t)v0 * 240 + e];
    for (int k = t; k <= n_k; k += PN_COOP_THREADS) kp_s[k] = kp_bg[k];
    for (int o = t; o < n3; o += PN_COOP_THREADS) Cs[o] = momentum[o] - rhs_rest[o];
    const bool ip_lane = t < nown * 8;
    const int vl = t >> 3, i8 = t & 7, v = v0 + vl;
    int kid = 0, cpos = 0;
    double m_ = 0.0, l_ = 0.0;
    // the warm-start rotations of the own integration points live in LDS between the iterations (18 registers of every thread otherwise)
    for (int e = t; e < nown * 9; e += PN_COOP_THREADS) Qs[e] = Vstore[(size_t)v0 * 9 + e];
    if (ip_lane) {
        kid = topo[v * 8 + i8];
        cpos = csr_pos[v * 8 + i8];
        if (i8 == 0) { m_ = mu[v]; l_ = lam[v]; }
    }
    // rows [r0, r0 + nrow) of A^-1: wave wid holds row r0 + wid, lane-strided (<= 8 rows per workgroup = its 8 waves)
    const int r0 = w * rpw, nrow = max(min(rpw, n - r0), 0);
    double Areg[CW];
#pragma unroll
    for (int u = 0; u < CW; u++) {
        const int j = lane + 64 * u;
        Areg[u] = (wid < nrow && j < n) ? Ainv[(size_t)(r0 + wid) * n + j] : 0.0;
    }
    const bool row_lane = wid < nrow && lane < 3;
    const double rest_o = row_lane ? dof_rest[(size_t)(r0 + wid) * 3 + lane] : 0.0, last_o = row_lane ? last[(size_t)(r0 + wid) * 3 + lane] : 0.0;
    // this workgroup's piece of a kernel's CSR list: slot ps (of 17) takes entries ps + 17 u, thread (ps, q) holds their dNx value q
    const int4 pc = w < n_pieces ? pieces[w] : make_int4(0, 0, 0, 0);  // (kernel, first entry, entries, -)
    const int p_bg = pc.y, p_cnt = pc.z;
    const int ps = t / 30, pq = t - ps * 30, pcq = pq / 10;
    const bool piece_lane = ps < PN_COOP_NS && p_cnt > 0;
    for (int e = t; e < p_cnt * 30; e += PN_COOP_THREADS) Gs[e] = dNx_csr[(size_t)p_bg * 30 + e];  // the piece's dNx rows, [entry][30]
    __syncthreads();
    PN_COOP_CLK(8);

    for (int it = 0; it < iters; it++) {
        // this iteration's exchange buffers (never read before in this launch, see ld_fresh)
        const double* dof_in = it == 0 ? dof : dofx_all + (size_t)(it - 1) * n3;
        double* dof_out = it == iters - 1 ? dof : dofx_all + (size_t)it * n3;
        double* psum = psum_all + (size_t)it * G * 30;
        // ================= integration points: F, warm-started SVD, stresses to the CSR positions of the eight neighbour kernels
        if (ip_lane) {
            double dv[30];
            if (fresh) {
#pragma unroll
                for (int q = 0; q < 30; q++) dv[q] = ld_fresh(dof_in + (size_t)kid * 30 + q);
            } else {
#pragma unroll
                for (int q = 0; q < 30; q++) dv[q] = ld_agent(dof_in + (size_t)kid * 30 + q);
            }
            const double* __restrict__ dn = Ds + (size_t)(vl * 8 + i8) * 30;
            M3 Fm;
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int c = 0; c < 3; c++) Fm.m[r][c] = 0.0;
#pragma unroll
            for (int x = 0; x < 10; x++) {
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const double gq = dn[c * 10 + x];
                    Fm.m[0][c] += dv[x * 3] * gq;
                    Fm.m[1][c] += dv[x * 3 + 1] * gq;
                    Fm.m[2][c] += dv[x * 3 + 2] * gq;
                }
            }
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    double sacc = Fm.m[r][c];
                    sacc += dpp_d<0xB1>(sacc);   // lanes ^ 1
                    sacc += dpp_d<0x4E>(sacc);   // lanes ^ 2
                    sacc += dpp_d<0x141>(sacc);  // the other quad of the 8-lane group (row_half_mirror)
                    Fm.m[r][c] = sacc;
                }
            double Pm[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
            if (i8 == 0) {
                M3 U, V;
                double sig[3], sp[3];
                if (dbg & 1) {  // timing experiment (PN_SIM_COOP_DBG=1): no SVD, results invalid
#pragma unroll
                    for (int r = 0; r < 3; r++)
#pragma unroll
                        for (int c = 0; c < 3; c++) { U.m[r][c] = (r == c); V.m[r][c] = (r == c); }
                    sig[0] = Fm.m[0][0]; sig[1] = Fm.m[1][1]; sig[2] = Fm.m[2][2];
                } else {
                    M3 Qw;
#pragma unroll
                    for (int r = 0; r < 3; r++)
#pragma unroll
                        for (int c = 0; c < 3; c++) Qw.m[r][c] = Qs[vl * 9 + r * 3 + c];
                    svd3(Fm, U, sig, V, &Qw, 1e-24);
#pragma unroll
                    for (int r = 0; r < 3; r++)
#pragma unroll
                        for (int c = 0; c < 3; c++) Qs[vl * 9 + r * 3 + c] = V.m[r][c];
                }
                volume_invariant_project(sig, sp);
#pragma unroll
                for (int r = 0; r < 3; r++)
#pragma unroll
                    for (int c = 0; c < 3; c++) {
                        const double R = U.m[r][0] * V.m[c][0] + U.m[r][1] * V.m[c][1] + U.m[r][2] * V.m[c][2];
                        const double Vv = U.m[r][0] * sp[0] * V.m[c][0] + U.m[r][1] * sp[1] * V.m[c][1] + U.m[r][2] * sp[2] * V.m[c][2];
                        Pm[r * 3 + c] = dx3 * (m_ * R + l_ * Vv);
                    }
            }
            const int src = lane & ~7;
            double* dst = P_csr + (size_t)cpos * 9;
#pragma unroll
            for (int q = 0; q < 9; q++) {
                int2 tt = *reinterpret_cast<int2*>(&Pm[q]);
                tt.x = __shfl(tt.x, src);
                tt.y = __shfl(tt.y, src);
                st_agent(dst + q, *reinterpret_cast<double*>(&tt));
            }
        }
        PN_COOP_CLK(0);
        if (!(dbg & 2) && !coop_sync(ctl, ++g, per_xcd, xcd)) return;
        PN_COOP_CLK(1);

        // ================= pieces: sum_e dNx_e^T P_e over this workgroup's piece (ascending entries per slot, slots in ascending order)
        if (p_cnt > 0) {
            double* Ps = Xs;
            {
                double pv[6];  // <= 272 * 9 / 512 loads per thread, all in flight
#pragma unroll
                for (int u = 0; u < 6; u++) {  // (unconditional, clamped: a branch around an atomic load makes the compiler wait for each one in turn)
                    const int e9 = min(t + PN_COOP_THREADS * u, p_cnt * 9 - 1);
                    pv[u] = ld_agent(P_csr + (size_t)p_bg * 9 + e9);
                }
#pragma unroll
                for (int u = 0; u < 6; u++) {
                    const int e9 = t + PN_COOP_THREADS * u;
                    if (e9 < p_cnt * 9) Ps[e9] = pv[u];
                }
            }
            __syncthreads();
            if (ps < PN_COOP_NS) {
                double a0 = 0.0, a1 = 0.0, a2 = 0.0;
#pragma unroll
                for (int u = 0; u < EU; u++) {
                    const int e = ps + PN_COOP_NS * u;
                    if (u < eu && e < p_cnt) {
                        const double* __restrict__ pe = Ps + (size_t)e * 9 + pcq;
                        const double gq = Gs[e * 30 + pq];
                        a0 += pe[0] * gq; a1 += pe[3] * gq; a2 += pe[6] * gq;
                    }
                }
                red[(ps * 30 + pq) * 3] = a0; red[(ps * 30 + pq) * 3 + 1] = a1; red[(ps * 30 + pq) * 3 + 2] = a2;
            }
            __syncthreads();
            if (t < 90) {  // (q, r): the 17 slots in order
                double sacc = 0.0;
#pragma unroll
                for (int sl = 0; sl < PN_COOP_NS; sl++) sacc += red[sl * 90 + t];
                red[t] = sacc;  // slot 0's own value was read by this thread only
            }
            __syncthreads();
            if (t < 30) {
                const int x = t / 3, r = t - x * 3;
                st_agent(psum + (size_t)w * 30 + t, (red[x * 3 + r] + red[(10 + x) * 3 + r]) + red[(20 + x) * 3 + r]);
            }
        }
        PN_COOP_CLK(2);
        if (!(dbg & 2) && !coop_sync(ctl, ++g, per_xcd, xcd)) return;
        PN_COOP_CLK(3);

        // ================= rows: right-hand side assembled in LDS (a kernel's pieces in ascending order), this workgroup's rows of A^-1 from registers
        {
            // every entry's first two pieces in ONE batch of unconditional loads (clamped addresses, selected afterwards), the third and fourth — a
            // few long lists have them — in a second, wave-uniform batch: a branch around an atomic load makes the compiler wait for each load in
            // turn, and nine dependent round trips per thread were 15 us of every iteration in the first version
            double pv[NO][2], sum[NO];
            int np[NO], pb[NO];
            bool more = false;
#pragma unroll
            for (int u = 0; u < NO; u++) {
                const int o = min(t + PN_COOP_THREADS * u, n3 - 1);
                const int k = o / 30, q = o - k * 30;
                pb[u] = kp_s[k];
                np[u] = kp_s[k + 1] - pb[u];
                const double* src = psum + (size_t)pb[u] * 30 + q;  // pb < n_wg always: a kernel without entries reads a neighbour's piece, unused
                if (fresh) { pv[u][0] = ld_fresh(src); pv[u][1] = ld_fresh(src + (np[u] > 1 ? 30 : 0)); }
                else { pv[u][0] = ld_agent(src); pv[u][1] = ld_agent(src + (np[u] > 1 ? 30 : 0)); }
                more |= np[u] > 2;
            }
#pragma unroll
            for (int u = 0; u < NO; u++) {
                sum[u] = np[u] > 0 ? pv[u][0] : 0.0;
                if (np[u] > 1) sum[u] += pv[u][1];
            }
            if (__builtin_amdgcn_ballot_w64(more) != 0ull) {
#pragma unroll
                for (int u = 0; u < NO; u++) {
                    const int o = min(t + PN_COOP_THREADS * u, n3 - 1);
                    const double* src = psum + (size_t)pb[u] * 30 + o % 30;
                    if (fresh) { pv[u][0] = ld_fresh(src + (np[u] > 2 ? 60 : 0)); pv[u][1] = ld_fresh(src + (np[u] > 3 ? 90 : 0)); }
                    else { pv[u][0] = ld_agent(src + (np[u] > 2 ? 60 : 0)); pv[u][1] = ld_agent(src + (np[u] > 3 ? 90 : 0)); }
                }
#pragma unroll
                for (int u = 0; u < NO; u++) {
                    if (np[u] > 2) sum[u] += pv[u][0];
                    if (np[u] > 3) sum[u] += pv[u][1];
                }
            }
#pragma unroll
            for (int u = 0; u < NO; u++) {
                const int o = t + PN_COOP_THREADS * u;
                if (o < n3) { const int j = o / 3, c = o - j * 3; Xs[c * n + j] = Cs[o] + sum[u]; }  // SoA by component: conflict-free reads in the row products
            }
        }
        __syncthreads();
        PN_COOP_CLK(4);
        if (wid < nrow) {  // wave wid = row r0 + wid: lane-strided columns from registers, X from LDS, one reduction of three values
            double a0 = 0.0, a1 = 0.0, a2 = 0.0;
#pragma unroll
            for (int u = 0; u < CW; u++) {
                const int j = lane + 64 * u;
                if (j < n) {
                    a0 += Areg[u] * Xs[j]; a1 += Areg[u] * Xs[n + j]; a2 += Areg[u] * Xs[2 * n + j];
                }
            }
            a0 = wave_sum_d(a0); a1 = wave_sum_d(a1); a2 = wave_sum_d(a2);
            if (lane < 3) {
                const double sacc = lane == 0 ? a0 : (lane == 1 ? a1 : a2);
                const size_t o = (size_t)(r0 + wid) * 3 + lane;
                const double dnew = rest_o + sacc;  // solver.py:601
                st_agent(dof_out + o, dnew);
                if (it == iters - 1) dof_vel[o] = (dnew - last_o) / dt * 0.998;  // solver.py:602 (k_step_end)
            }
        }
        PN_COOP_CLK(5);
        if (it < iters - 1 && !(dbg & 2) && !coop_sync(ctl, ++g, per_xcd, xcd)) return;
        PN_COOP_CLK(6);
    }
    if (clk_on) for (int i = 0; i < 9; i++) reinterpret_cast<unsigned long long*>(ctl->err + 8)[i] += clk_s[i];
#undef PN_COOP_CLK
    __syncthreads();
    for (int e = t; e < nown * 9; e += PN_COOP_THREADS) Vstore[(size_t)v0 * 9 + e] = Qs[e];
}

extern "C" uint64_t pn_sim_coop_bytes(int n_k, int n_IP, int n_wg) {
    PnCoopPlan pl;
    if (n_k <= 0 || n_IP <= 0 || !pn_coop_plan(n_k, n_IP, n_wg, nullptr, &pl)) return 0;
    return pl.bytes;
}

// Lays out the pieces (host side: reads csr_cnt back once) and clears the barrier state.  Returns PN_ERR_ARG when the scene does not fit the
// persistent form (more than 2048 unknowns per component, lists too long for n_wg register-resident pieces, LDS) — the caller keeps the launch form.
extern "C" int pn_sim_coop_prepare(int n_k, int n_IP, int n_wg, const int* csr_bg, const int* csr_cnt, void* coop, int* plan_out, void* stream) {
    PN_REQUIRE(n_k > 0 && n_IP > 0 && csr_bg && csr_cnt && coop && plan_out);
    hipStream_t st = (hipStream_t)stream;
    std::vector<int> cnt(n_k), bg(n_k);
    PN_HIP_CHECK(hipMemcpyAsync(cnt.data(), csr_cnt, (size_t)n_k * sizeof(int), hipMemcpyDeviceToHost, st));
    PN_HIP_CHECK(hipMemcpyAsync(bg.data(), csr_bg, (size_t)n_k * sizeof(int), hipMemcpyDeviceToHost, st));
    PN_HIP_CHECK(hipStreamSynchronize(st));
    PnCoopPlan pl;
    PN_REQUIRE(pn_coop_plan(n_k, n_IP, n_wg, cnt.data(), &pl));
    PN_REQUIRE(pl.max_pieces_per_kernel <= PN_COOP_MAXP);
    std::vector<unsigned char> img(pl.bytes, 0);
    int4* pieces = reinterpret_cast<int4*>(img.data() + pl.off_pieces);
    int* kp = reinterpret_cast<int*>(img.data() + pl.off_kp);
    const int pmax = pl.eu * PN_COOP_NS;
    int np = 0;
    for (int k = 0; k < n_k; k++) {
        kp[k] = np;
        for (int b = 0; b < cnt[k]; b += pmax) pieces[np++] = make_int4(k, bg[k] + b, std::min(pmax, cnt[k] - b), b / pmax);
    }
    kp[n_k] = np;
    PN_REQUIRE(np == pl.n_pieces);
    PN_HIP_CHECK(hipMemcpyAsync(coop, img.data(), pl.bytes, hipMemcpyHostToDevice, st));
    PN_HIP_CHECK(hipStreamSynchronize(st));
    plan_out[0] = pl.n_pieces;
    plan_out[1] = pl.eu;
    plan_out[2] = pl.max_pieces_per_kernel;
    return PN_OK;
}

// 0: no launch of this buffer has timed out at a barrier; 1: one has (its results are invalid; pn_sim_coop_prepare again before reuse).  Synchronous.
extern "C" int pn_sim_coop_status(const void* coop, int* timed_out) {
    PN_REQUIRE(coop && timed_out);
    PN_HIP_CHECK(hipMemcpy(timed_out, reinterpret_cast<const PnCoopCtl*>(coop)->err, sizeof(int), hipMemcpyDeviceToHost));
    return PN_OK;
}

// Timing experiments (PN_SIM_COOP_DBG & 4): the nine tick accumulators of workgroup 0 (integration points, exchange, pieces, exchange, assembly,
// rows, exchange, -, kernel start), 100 MHz ticks summed over all launches since pn_sim_coop_prepare.
extern "C" int pn_sim_coop_clocks(const void* coop, uint64_t* ticks9) {
    PN_REQUIRE(coop && ticks9);
    PN_HIP_CHECK(hipMemcpy(ticks9, reinterpret_cast<const PnCoopCtl*>(coop)->err + 8, 9 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return PN_OK;
}

extern "C" int pn_sim_stepforward_coop(int n_k, int n_IP, int iters, double dt, double dx, const int* topo, const double* mu, const double* lam,
                                       const double* dNx, const double* dNx_csr, const int* csr_pos, const double* Ainv, const double* Mmat,
                                       const double* dof_rest, const double* rhs_rest, const double* rhs_gravity, const double* dof_f, double* dof,
                                       double* dof_vel, double* work, void* coop, int n_wg, const int* plan, void* stream) {
    PN_REQUIRE(n_k > 0 && n_IP > 0 && iters >= 1 && iters <= PN_COOP_ITERS && topo && mu && lam && dNx && dNx_csr && csr_pos && Ainv && Mmat);
    PN_REQUIRE(dof_rest && rhs_rest && rhs_gravity && dof_f && dof && dof_vel && work && coop);
    hipStream_t st = (hipStream_t)stream;
    PnCoopPlan pl;
    PN_REQUIRE(plan);
    const int n_pieces = plan[0], eu = plan[1], max_rank = plan[2];
    PN_REQUIRE(n_pieces > 0 && n_pieces <= n_wg && eu >= 1 && eu <= PN_COOP_EU && max_rank >= 1 && max_rank <= PN_COOP_MAXP);
    PN_REQUIRE(pn_coop_plan(n_k, n_IP, n_wg, nullptr, &pl, eu));
    const int n = n_k * 10, n3 = n * 3;
    double* tilde = work;
    double* last = work + n3;
    double* momentum = work + 2 * (size_t)n3;
    double* P_csr = work + 4 * (size_t)n3 + (size_t)n_IP * 9;
    double* Vstore = pn_sim_vstore(work, n_k, n_IP);
    unsigned char* cb = reinterpret_cast<unsigned char*>(coop);
    // the smallest register-resident shape that holds this scene
    const int cw = (n + 63) / 64, no = (n3 + PN_COOP_THREADS - 1) / PN_COOP_THREADS;
    const bool small = cw <= 22 && no <= 9;
    auto kern = small ? k_substep_coop<22, PN_COOP_EU, 9> : k_substep_coop<PN_COOP_CU * 8, PN_COOP_EU, PN_COOP_CU * 3>;
    if (pl.lds_bytes > 48 * 1024) {  // dynamic LDS above 48 KB is opted into per device (and per function)
        static size_t granted[2][PN_MAX_DEVICES] = {{0}, {0}};
        int dev_id = 0;
        PN_HIP_CHECK(hipGetDevice(&dev_id));
        if (dev_id < 0 || dev_id >= PN_MAX_DEVICES || pl.lds_bytes > granted[small][dev_id]) {
            PN_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds_bytes));
            if (dev_id >= 0 && dev_id < PN_MAX_DEVICES) granted[small][dev_id] = pl.lds_bytes;
        }
    }
    k_step_begin<<<pn_div_up(n3, 256), 256, 0, st>>>(n3, dt, dof, dof_vel, tilde, last, reinterpret_cast<int*>(cb));
    k_matvec3<<<pn_div_up(n, 8), 256, 0, st>>>(n, Mmat, tilde, momentum, 1, dof_f, rhs_gravity);  // compute_momentum (:574-576)
    kern<<<n_wg, PN_COOP_THREADS, pl.lds_bytes, st>>>(n_k, n_IP, iters, dt, pow(dx, 3.0), topo, csr_pos, mu, lam, dNx, dNx_csr, Ainv, dof_rest, rhs_rest, momentum, last,
                                                      dof, dof_vel, P_csr, Vstore, reinterpret_cast<PnCoopCtl*>(cb), reinterpret_cast<const int4*>(cb + pl.off_pieces),
                                                      reinterpret_cast<const int*>(cb + pl.off_kp), reinterpret_cast<double*>(cb + pl.off_psum), reinterpret_cast<double*>(cb + pl.off_dofx), n_pieces, eu,
                                                      pl.ipw, pl.rpw, max_rank, (int)pn_env_u32("PN_SIM_COOP_DBG", 0));
    PN_LAUNCH_CHECK();
    return PN_OK;
}

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

// ------------------------------------------------------------------------------------------------ misc
extern "C" int pn_device_cu_count(void) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess) return -1;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return -1;
    return n;
}

extern "C" int pn_stream_create_cu_mask(uint32_t total_cu, uint32_t first_cu, uint32_t n_cu, int invert, void** stream_out) {
    PN_REQUIRE(stream_out && total_cu > 0 && total_cu <= 1024 && n_cu > 0 && first_cu + n_cu <= total_cu);
    uint32_t mask[32];
    const uint32_t words = (total_cu + 31) / 32;
    for (uint32_t w = 0; w < words; w++) mask[w] = 0;
    for (uint32_t i = 0; i < total_cu; i++) {
        const bool in = i >= first_cu && i < first_cu + n_cu;
        if (in != (invert != 0)) mask[i / 32] |= 1u << (i % 32);
    }
    hipStream_t s = nullptr;
    PN_HIP_CHECK(hipExtStreamCreateWithCUMask(&s, words, mask));
    *stream_out = (void*)s;
    return PN_OK;
}

extern "C" int pn_stream_destroy(void* stream) {
    PN_REQUIRE(stream);
    PN_HIP_CHECK(hipStreamDestroy((hipStream_t)stream));
    return PN_OK;
}

extern "C" const char* pn_version(void) { return "pienerf_hip 0.1.0 gfx950"; }
extern "C" const char* pn_last_error(void) { return pn_err_buf; }
