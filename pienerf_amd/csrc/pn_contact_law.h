// One collider's part of the contact law (include/pienerf_hip.h: pn_contact_state), shared by contact (pn_contact.hip: every collider, at an
// integration point) and the rigid balls (pn_bodies.hip: one dynamic slot at an integration point for the reaction; the static colliders at a ball's
// centre, its radius in the thickness's place).  One source for these lines, and the contraction flag the two units share, make a point's term from
// slot b the same bits on the object's side and in the reaction.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "pn_common.h"

// a += a_n nh - a_t w_t / |w_t| for the collider `col` at a point x with velocity v and thickness h; returns whether it is penetrated (delta > 0), and
// then delta in *delta_out.  A collider with delta = 0, and an empty slot, add exactly nothing and leave *delta_out alone.
__device__ __forceinline__ bool pn_contact_collider_term(const pn_contact_collider* __restrict__ col, double kappa, double beta, double mu, double h, double dt,
                                                         double dt2, const double x[3], const double v[3], double a[3], double* delta_out) {
    const int type = col->type;
    if (type < PN_CONTACT_PLANE || type > PN_CONTACT_CAPSULE) return false;
    double nh[3], d;
    double r0 = x[0] - col->p[0], r1 = x[1] - col->p[1], r2 = x[2] - col->p[2];
    if (type == PN_CONTACT_PLANE) {
        nh[0] = col->n[0]; nh[1] = col->n[1]; nh[2] = col->n[2];
        d = nh[0] * r0 + nh[1] * r1 + nh[2] * r2;
    } else if (type == PN_CONTACT_BOX) {  // n: the half-extents
        const double q0 = fabs(r0) - col->n[0], q1 = fabs(r1) - col->n[1], q2 = fabs(r2) - col->n[2];
        const double s0 = r0 >= 0.0 ? 1.0 : -1.0, s1 = r1 >= 0.0 ? 1.0 : -1.0, s2 = r2 >= 0.0 ? 1.0 : -1.0;
        if (fmax(fmax(q0, q1), q2) > 0.0) {  // outside: the Euclidean distance to the face, edge or corner
            const double e0 = fmax(q0, 0.0), e1 = fmax(q1, 0.0), e2 = fmax(q2, 0.0);
            d = sqrt(e0 * e0 + e1 * e1 + e2 * e2);
            nh[0] = s0 * e0 / d; nh[1] = s1 * e1 / d; nh[2] = s2 * e2 / d;
        } else {  // inside or on the surface: the nearest face, the lowest axis on ties
            nh[0] = nh[1] = nh[2] = 0.0;
            if (q0 >= q1 && q0 >= q2) { d = q0; nh[0] = s0; }
            else if (q1 >= q2) { d = q1; nh[1] = s1; }
            else { d = q2; nh[2] = s2; }
        }
    } else {
        if (type == PN_CONTACT_CAPSULE) {  // n = B - A: the sphere's rule about the segment's closest point c = p + s n
            const double n0 = col->n[0], n1 = col->n[1], n2 = col->n[2];
            const double s = fmin(fmax((r0 * n0 + r1 * n1 + r2 * n2) / (n0 * n0 + n1 * n1 + n2 * n2), 0.0), 1.0);
            r0 = x[0] - (col->p[0] + s * n0); r1 = x[1] - (col->p[1] + s * n1); r2 = x[2] - (col->p[2] + s * n2);
        }
        const double L = sqrt(r0 * r0 + r1 * r1 + r2 * r2);
        if (L > 0.0) {
            nh[0] = r0 / L; nh[1] = r1 / L; nh[2] = r2 / L;
        } else {
            nh[0] = 0.0; nh[1] = 1.0; nh[2] = 0.0;
        }
        d = L - col->R;
        if (type == PN_CONTACT_CONTAINER) {
            d = -d;
            nh[0] = -nh[0]; nh[1] = -nh[1]; nh[2] = -nh[2];
        }
    }
    // from here on the lines are restated in pn_contact_response below (the signed-distance grids): a change to either goes into both
    const double delta = h - d;
    if (!(delta > 0.0)) return false;
    *delta_out = delta;
    const double w0 = v[0] - col->v[0], w1 = v[1] - col->v[1], w2 = v[2] - col->v[2];
    const double wn = w0 * nh[0] + w1 * nh[1] + w2 * nh[2];
    const double t0 = w0 - wn * nh[0], t1 = w1 - wn * nh[1], t2 = w2 - wn * nh[2];
    const double an = (kappa * delta + beta * fmin(fmax(-wn, 0.0) * dt, delta)) / dt2;
    a[0] += an * nh[0]; a[1] += an * nh[1]; a[2] += an * nh[2];
    const double wt = sqrt(t0 * t0 + t1 * t1 + t2 * t2);
    if (wt > 0.0) {
        const double at = fmin(mu * an, wt / dt), s = at / wt;
        a[0] -= s * t0; a[1] -= s * t1; a[2] -= s * t2;
    }
    return true;
}

// The same response for a solid given by a signed distance d and a unit normal nh alone (the signed-distance grids of pn_sdf.hip), moving with
// velocity cv: the lines of pn_contact_collider_term from `delta` on, restated here rather than shared with it so that the analytic colliders' code,
// and with it their bits, stay what they were.  delta = 0 adds exactly nothing and leaves *delta_out alone.
__device__ __forceinline__ bool pn_contact_response(const double nh[3], double d, const double cv[3], double kappa, double beta, double mu, double h, double dt,
                                                    double dt2, const double v[3], double a[3], double* delta_out) {
    const double delta = h - d;
    if (!(delta > 0.0)) return false;
    *delta_out = delta;
    const double w0 = v[0] - cv[0], w1 = v[1] - cv[1], w2 = v[2] - cv[2];
    const double wn = w0 * nh[0] + w1 * nh[1] + w2 * nh[2];
    const double t0 = w0 - wn * nh[0], t1 = w1 - wn * nh[1], t2 = w2 - wn * nh[2];
    const double an = (kappa * delta + beta * fmin(fmax(-wn, 0.0) * dt, delta)) / dt2;
    a[0] += an * nh[0]; a[1] += an * nh[1]; a[2] += an * nh[2];
    const double wt = sqrt(t0 * t0 + t1 * t1 + t2 * t2);
    if (wt > 0.0) {
        const double at = fmin(mu * an, wt / dt), s = at / wt;
        a[0] -= s * t0; a[1] -= s * t1; a[2] -= s * t2;
    }
    return true;
}
