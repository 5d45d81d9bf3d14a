// The simulator's 3x3 decompositions and the small fp64 helpers around them (included by pn_sim.hip only).
#pragma once
#include "pn_common.h"

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

// A lane's share of an integration point's deformation gradient, shared by every form of the substep (k_elastic, k_cells_elastic_gather, k_substep_coop):
// F[r][c] += d[x * 3 + r] * g[c * 10 + x] over its neighbour kernel's 10 coefficients (d: the kernel's DOFs, g: this point's shape-function gradients for
// that kernel; registers, global memory or LDS), x outer and c inner.  The sum over the point's 8 lanes (lanes ^1, ^2, ^4 in every form) stays with each
// kernel.  (The stress from U, sig, V is still written out per kernel: shared, it changed which products the backend fuses, and with it the bits.)
__device__ __forceinline__ void ip_F_partial(const double* d, const double* g, M3& F) {
#pragma unroll
    for (int x = 0; x < 10; x++)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const double gg = g[c * 10 + x];
            F.m[0][c] += d[x * 3] * gg;
            F.m[1][c] += d[x * 3 + 1] * gg;
            F.m[2][c] += d[x * 3 + 2] * gg;
        }
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
