// The contact colliders drawn into a rendered frame (include/pienerf_hip.h: pn_draw_colliders has the law).
//
// pn_draw_colliders_shadowed is the same launch with the object's shadow looked up while it draws: both kernels are pn_draw_ray, built
// from the same device functions, and the unshadowed one keeps its bits.
//
// The colliders are analytic surfaces in the world space of the rays, and a finished frame carries what a depth-tested composite needs per ray
// (weights_sum, depth_0), so this is one per-ray launch behind the frame driver, as the background model's blend is (pn_background.hip).  The state is
// read on the device: a launch captured into a HIP graph draws the colliders where set_collider last put them.  Built with -ffp-contract=off: every
// operation rounds once, in the order written here, which tests/colliders_reference.py restates in numpy.
#include <math.h>

#include "pn_common.h"

static_assert(sizeof(pn_collider_style) == 108, "pn_collider_style: 27 floats (pienerf_amd/_lib.py: ColliderStyle)");
static_assert(sizeof(pn_shadow_light) == 72, "pn_shadow_light: 18 four-byte members (pienerf_amd/_lib.py: ShadowLight)");
static_assert(PN_CONTACT_SLOTS == 8, "pn_collider_style.rgb: one colour per collider slot");

#define PN_COLLIDER_THREADS 256

// A slot as the rays read it: the state's fp64 fields rounded to fp32, and a plane's tangent frame, once per workgroup.  A capsule keeps its unit
// axis in u, its end point B = p + n in v and the axis's length in len; a box's n are its half-extents.
struct PnDrawSlot {
    int type;
    float p[3], n[3], R;
    float u[3], v[3];
    float rgb[3];
    float len;
};

__device__ __forceinline__ float pn_dot3(const float a[3], const float b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// The slots as the rays read them, by the workgroup's first PN_CONTACT_SLOTS threads; the caller's barrier follows.
// *s_new: whether a slot holds a box or a capsule, by a ballot of the first wave.
__device__ __forceinline__ void pn_load_slot(const pn_contact_state* __restrict__ st, const pn_collider_style& style, int tid, PnDrawSlot* s_slot, int* s_n,
                                             int* s_new) {
    if (tid < 64) {
        const int type = tid < PN_CONTACT_SLOTS ? st->c[tid].type : PN_CONTACT_EMPTY;
        const bool any_new = __any(type == PN_CONTACT_BOX || type == PN_CONTACT_CAPSULE) != 0;
        if (tid == 0) *s_new = any_new ? 1 : 0;
    }
    if (tid < PN_CONTACT_SLOTS) {
        const pn_contact_collider* c = st->c + tid;
        PnDrawSlot* s = s_slot + tid;
        const int type = c->type;
        s->type = (type >= PN_CONTACT_PLANE && type <= PN_CONTACT_CAPSULE) ? type : PN_CONTACT_EMPTY;
        float n[3];
        for (int i = 0; i < 3; i++) {
            s->p[i] = (float)c->p[i];
            s->n[i] = n[i] = (float)c->n[i];
            s->rgb[i] = style.rgb[tid][i];
        }
        s->R = (float)c->R;
        s->len = 0.0f;
        if (type == PN_CONTACT_CAPSULE) {   // unit axis n / |n|, B = p + n; an axis that vanishes in fp32 leaves the solid sphere about A
            const float len = sqrtf(pn_dot3(n, n));
            if (!(len > 0.0f)) s->type = PN_CONTACT_SPHERE;
            for (int i = 0; i < 3; i++) {
                s->u[i] = len > 0.0f ? n[i] / len : 0.0f;
                s->v[i] = s->p[i] + n[i];
            }
            s->len = len;
            if (tid == 0) *s_n = min(max(st->n, 0), PN_CONTACT_SLOTS);
            return;
        }
        // the checker's frame: u = normalised n x e, e the axis on which |n| is smallest (lowest index on ties), v = n x u
        const float a0 = fabsf(n[0]), a1 = fabsf(n[1]), a2 = fabsf(n[2]);
        float u[3];
        if (a0 <= a1 && a0 <= a2) { u[0] = 0.0f; u[1] = n[2]; u[2] = -n[1]; }
        else if (a1 <= a2) { u[0] = -n[2]; u[1] = 0.0f; u[2] = n[0]; }
        else { u[0] = n[1]; u[1] = -n[0]; u[2] = 0.0f; }
        const float L = sqrtf(pn_dot3(u, u));
        for (int i = 0; i < 3; i++) u[i] = L > 0.0f ? u[i] / L : 0.0f;
        s->u[0] = u[0]; s->u[1] = u[1]; s->u[2] = u[2];
        s->v[0] = n[1] * u[2] - n[2] * u[1];
        s->v[1] = n[2] * u[0] - n[0] * u[2];
        s->v[2] = n[0] * u[1] - n[1] * u[0];
        if (tid == 0) *s_n = min(max(st->n, 0), PN_CONTACT_SLOTS);
    }
}

// The interval (t_enter, t_exit) in which the ray o + t d is inside the box (centre p, half-extents h), by the three slabs, and the axes that gave
// the two ends (the lowest index on ties): a hit iff t_enter < t_exit.  A ray parallel to a slab is inside it for all t or misses.
__device__ __forceinline__ bool pn_box_interval(const float* p, const float* h, const float o[3], const float d[3], float* t_enter, float* t_exit,
                                                int* f_enter, int* f_exit) {
    float te = -INFINITY, tx = INFINITY;
    int fe = -1, fx = -1;
    bool inside = true;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        if (d[i] == 0.0f) {
            if (!(fabsf(o[i] - p[i]) < h[i])) inside = false;
        } else {
            const float t1 = ((p[i] - h[i]) - o[i]) / d[i], t2 = ((p[i] + h[i]) - o[i]) / d[i];
            const float lo = fminf(t1, t2), hi = fmaxf(t1, t2);
            if (lo > te) { te = lo; fe = i; }
            if (hi < tx) { tx = hi; fx = i; }
        }
    }
    *t_enter = te; *t_exit = tx; *f_enter = fe; *f_exit = fx;
    return inside && te < tx;
}

// The roots of a sphere (centre c, radius R) along o + t d, q = d.d: the sphere branch of pn_find_hit, for a capsule's ends.
__device__ __forceinline__ bool pn_sphere_interval(const float* c, float R, const float o[3], const float d[3], float q, float* t_near, float* t_far) {
    const float oc[3] = {o[0] - c[0], o[1] - c[1], o[2] - c[2]};
    const float b = pn_dot3(oc, d);
    const float disc = b * b - q * (pn_dot3(oc, oc) - R * R);
    if (!(disc > 0.0f)) return false;
    const float sq = sqrtf(disc);
    *t_near = (-b - sq) / q;
    *t_far = (-b + sq) / q;
    return true;
}

// The interval in which the ray is inside the capsule `c`: the convex union of the two end spheres and the finite cylinder between them — the smallest
// near and the largest far over the parts that are hit.  The cylinder: with a the unit axis, oc = o - A, ad = a.d, ao = a.oc, dp = d - ad a,
// op = oc - ao a:  A2 = dp.dp, b = op.dp, disc = b b - A2 (op.op - R R);  hit iff A2 > 0 and disc > 0, roots (-b -+ sqrt(disc)) / A2, intersected with
// the slab 0 < ao + t ad < len (ad == 0: the whole line or nothing), kept iff near < far.
__device__ __forceinline__ bool pn_capsule_interval(const PnDrawSlot* c, const float o[3], const float d[3], float q, float* t_near, float* t_far) {
    float tn = INFINITY, tf = -INFINITY, a, b;
    bool hit = false;
    if (pn_sphere_interval(c->p, c->R, o, d, q, &a, &b)) { tn = a; tf = b; hit = true; }
    if (pn_sphere_interval(c->v, c->R, o, d, q, &a, &b)) { tn = fminf(tn, a); tf = fmaxf(tf, b); hit = true; }
    const float oc[3] = {o[0] - c->p[0], o[1] - c->p[1], o[2] - c->p[2]};
    const float ad = pn_dot3(c->u, d), ao = pn_dot3(c->u, oc);
    const float dp[3] = {d[0] - ad * c->u[0], d[1] - ad * c->u[1], d[2] - ad * c->u[2]};
    const float op[3] = {oc[0] - ao * c->u[0], oc[1] - ao * c->u[1], oc[2] - ao * c->u[2]};
    const float A2 = pn_dot3(dp, dp);
    const float bc = pn_dot3(op, dp);
    const float disc = bc * bc - A2 * (pn_dot3(op, op) - c->R * c->R);
    if (A2 > 0.0f && disc > 0.0f) {
        const float sq = sqrtf(disc);
        float lo = (-bc - sq) / A2, hi = (-bc + sq) / A2;
        bool in = true;
        if (ad == 0.0f) {
            in = ao > 0.0f && ao < c->len;
        } else {
            const float s1 = (0.0f - ao) / ad, s2 = (c->len - ao) / ad;
            lo = fmaxf(lo, fminf(s1, s2));
            hi = fminf(hi, fmaxf(s1, s2));
        }
        if (in && lo < hi) { tn = fminf(tn, lo); tf = fmaxf(tf, hi); hit = true; }
    }
    *t_near = tn; *t_far = tf;
    return hit;
}

// The nearest slot the ray hits in (t_min, t_max), a later slot winning only with a strictly smaller t: its index (-1: none), t (+inf) and, for a
// box, the axis of the face that was hit.  NEW: the state holds a box or a capsule (uniform over the launch); without it the code is the planes' and
// spheres' as it has always been, and a frame of those alone runs exactly that.
template <bool NEW>
__device__ __forceinline__ int pn_find_hit(const PnDrawSlot* s_slot, int n_slots, const float o[3], const float d[3], float q, float t_min, float t_max,
                                           float* t_out, int* face_out) {
    float t_hit = INFINITY;
    int k_hit = -1, face_hit = 0;
    for (int k = 0; k < n_slots; k++) {   // the slot's type is uniform over the workgroup: no lane diverges on it
        const PnDrawSlot* c = s_slot + k;
        const int type = c->type;
        if (type == PN_CONTACT_EMPTY) continue;
        float t;
        int face = 0;
        if (type == PN_CONTACT_PLANE) {
            const float nd = pn_dot3(c->n, d);
            if (!(nd < 0.0f)) continue;   // front face only
            const float po[3] = {c->p[0] - o[0], c->p[1] - o[1], c->p[2] - o[2]};
            t = pn_dot3(c->n, po) / nd;
        } else if (NEW && type == PN_CONTACT_BOX) {
            float t_enter, t_exit;
            int f_enter, f_exit;
            if (!pn_box_interval(c->p, c->n, o, d, &t_enter, &t_exit, &f_enter, &f_exit)) continue;
            t = t_exit; face = f_exit;   // the eye inside: the far face
            if (t_enter > t_min) { t = t_enter; face = f_enter; }
        } else if (NEW && type == PN_CONTACT_CAPSULE) {
            float t_near, t_far;
            if (!pn_capsule_interval(c, o, d, q, &t_near, &t_far)) continue;
            t = t_far;
            if (t_near > t_min) t = t_near;
        } else {
            const float oc[3] = {o[0] - c->p[0], o[1] - c->p[1], o[2] - c->p[2]};
            const float b = pn_dot3(oc, d);
            const float disc = b * b - q * (pn_dot3(oc, oc) - c->R * c->R);
            if (!(disc > 0.0f)) continue;
            const float sq = sqrtf(disc);
            const float t_far = (-b + sq) / q;
            t = t_far;
            if (type == PN_CONTACT_SPHERE) {
                const float t_near = (-b - sq) / q;
                if (t_near > t_min) t = t_near;
            }
        }
        if (!(t > t_min && t < t_max)) continue;
        if (t < t_hit) { t_hit = t; k_hit = k; face_hit = face; }
    }
    *t_out = t_hit;
    *face_out = face_hit;
    return k_hit;
}

// The hit point x = o + t d and the hit slot's colour there: (rgb factor) shade.  `face`: a box's hit axis (pn_find_hit).
template <bool NEW>
__device__ __forceinline__ void pn_hit_colour(const PnDrawSlot* c, const pn_collider_style& style, const float o[3], const float d[3], float q, float t,
                                              int face, float x[3], float col[3]) {
    for (int j = 0; j < 3; j++) x[j] = o[j] + t * d[j];
    const float r[3] = {x[0] - c->p[0], x[1] - c->p[1], x[2] - c->p[2]};
    float factor = 1.0f, nd;
    if (c->type == PN_CONTACT_PLANE) {
        nd = pn_dot3(c->n, d);
        if (style.checker > 0.0f) {
            const float cells = floorf(pn_dot3(c->u, r) / style.checker) + floorf(pn_dot3(c->v, r) / style.checker);
            const float half = cells * 0.5f;   // parity without an integer conversion: exact below 2^24 cells, even beyond
            if (half != floorf(half)) factor = style.checker_dim;
        }
    } else if (NEW && c->type == PN_CONTACT_BOX) {   // the normal is the face's axis (its sign drops out of |n.d|); the checker over the other two axes
        nd = face == 0 ? d[0] : (face == 1 ? d[1] : d[2]);
        if (style.checker > 0.0f) {
            const float ra = face == 0 ? r[1] : r[0], rb = face == 2 ? r[1] : r[2];
            const float cells = floorf(ra / style.checker) + floorf(rb / style.checker);
            const float half = cells * 0.5f;
            if (half != floorf(half)) factor = style.checker_dim;
        }
    } else if (NEW && c->type == PN_CONTACT_CAPSULE) {   // the sphere's normal about the segment's closest point A + clamp(a.r, 0, len) a
        const float hc = fminf(fmaxf(pn_dot3(c->u, r), 0.0f), c->len);
        const float nrm[3] = {(r[0] - hc * c->u[0]) / c->R, (r[1] - hc * c->u[1]) / c->R, (r[2] - hc * c->u[2]) / c->R};
        nd = pn_dot3(nrm, d);
    } else {
        const float nrm[3] = {r[0] / c->R, r[1] / c->R, r[2] / c->R};   // the container's sign drops out of |n.d|
        nd = pn_dot3(nrm, d);
    }
    const float shade = style.ambient + (1.0f - style.ambient) * (fabsf(nd) / sqrtf(q));
    for (int j = 0; j < 3; j++) col[j] = c->rgb[j] * factor * shade;
}

// The depth-tested composite of a hit of colour `col` at t over the frame's (acc, s, d0); returns the coverage.
__device__ __forceinline__ float pn_composite_hit(const float col[3], float t, float t_max, const float acc[3], float s, float d0, float out[3]) {
    const float a = fminf(fmaxf((t_max - t) / (0.5f * t_max), 0.0f), 1.0f);
    const float t_obj = s > 1e-4f ? d0 / s : INFINITY;
    if (t < t_obj) {   // in front of the object
        for (int j = 0; j < 3; j++) out[j] = a * col[j] + (1.0f - a) * acc[j];
        return a + (1.0f - a) * s;
    }
    const float w = (1.0f - s) * a;   // behind it
    for (int j = 0; j < 3; j++) out[j] = acc[j] + w * col[j];
    return s + w;
}

// How much of the light the hit point x of slot k_hit loses (include/pienerf_hip.h: pn_draw_colliders_shadowed has the law): the object's opacity map
// seen from the light, four texels with a depth test each, and the solid spheres, boxes and capsules other than k_hit.  Every index is range-checked in float before it
// is converted: a point outside the map, or a non-finite coordinate, reads nothing.
template <bool NEW>
__device__ __forceinline__ float pn_shadow_occlusion(const pn_shadow_light& lt, const float* __restrict__ shadow_ws, const float* __restrict__ shadow_depth_0,
                                                     const PnDrawSlot* s_slot, int n_slots, int k_hit, const float x[3]) {
    const float r[3] = {x[0] - lt.c[0], x[1] - lt.c[1], x[2] - lt.c[2]};
    const float u = pn_dot3(lt.U, r), v = pn_dot3(lt.V, r), w = pn_dot3(lt.L, r);
    const float t_r = lt.D - w;
    const float Sf = (float)lt.S;
    const float scale = Sf / (2.0f * lt.half);
    const float fu = (u + lt.half) * scale - 0.5f, fv = (v + lt.half) * scale - 0.5f;
    const float i0 = floorf(fu), j0 = floorf(fv);
    const float au = fu - i0, av = fv - j0;
    float sum = 0.0f;
    for (int dj = 0; dj < 2; dj++) {
        for (int di = 0; di < 2; di++) {
            const float fi = i0 + (float)di, fj = j0 + (float)dj;
            if (!(fi >= 0.0f && fi < Sf && fj >= 0.0f && fj < Sf)) continue;
            const int idx = (int)fj * lt.S + (int)fi;
            const float sm = shadow_ws[idx];
            const float t_o = sm > 1e-4f ? shadow_depth_0[idx] / sm : INFINITY;
            if (t_r > t_o + lt.bias) sum = sum + ((di ? au : 1.0f - au) * (dj ? av : 1.0f - av)) * sm;
        }
    }
    const float occ_map = fminf(fmaxf(sum, 0.0f), 1.0f);
    float occ_sph = 0.0f;
    if (lt.spheres) {
        for (int k = 0; k < n_slots; k++) {
            const PnDrawSlot* c = s_slot + k;
            if (k == k_hit) continue;
            if (NEW && c->type == PN_CONTACT_BOX) {   // the light ray x + s L, s > 0, passes through the solid: pn_find_hit's intervals, far end > 0
                float t_enter, t_exit;
                int f_enter, f_exit;
                if (pn_box_interval(c->p, c->n, x, lt.L, &t_enter, &t_exit, &f_enter, &f_exit) && t_exit > 0.0f) occ_sph = 1.0f;
                continue;
            }
            if (NEW && c->type == PN_CONTACT_CAPSULE) {
                float t_near, t_far;
                if (pn_capsule_interval(c, x, lt.L, pn_dot3(lt.L, lt.L), &t_near, &t_far) && t_far > 0.0f) occ_sph = 1.0f;
                continue;
            }
            if (c->type != PN_CONTACT_SPHERE) continue;
            const float oc[3] = {x[0] - c->p[0], x[1] - c->p[1], x[2] - c->p[2]};
            const float b = pn_dot3(oc, lt.L);
            const float disc = b * b - (pn_dot3(oc, oc) - c->R * c->R);
            if (disc > 0.0f && -b + sqrtf(disc) > 0.0f) occ_sph = 1.0f;
        }
    }
    return fmaxf(occ_map, occ_sph);
}

// One ray's hit search, colour, shadow and composite: out, *cov, *occ and *t_hit.  NEW as in pn_find_hit.
template <bool SHADOWED, bool NEW>
__device__ __forceinline__ void pn_trace_ray(const PnDrawSlot* s_slot, int n_slots, const pn_collider_style& style, const float o[3], const float d[3], float q,
                                             float t_min, float t_max, const float acc[3], float s, float d0, const pn_shadow_light& lt,
                                             const float* __restrict__ shadow_ws, const float* __restrict__ shadow_depth_0, float out[3], float* cov,
                                             float* occ, float* t_out) {
    float t_hit;
    int face;
    const int k_hit = pn_find_hit<NEW>(s_slot, n_slots, o, d, q, t_min, t_max, &t_hit, &face);
    if (k_hit >= 0) {
        float x[3], col[3];
        pn_hit_colour<NEW>(s_slot + k_hit, style, o, d, q, t_hit, face, x, col);
        if (SHADOWED) {
            *occ = pn_shadow_occlusion<NEW>(lt, shadow_ws, shadow_depth_0, s_slot, n_slots, k_hit, x);
            const float lit = 1.0f - lt.strength * *occ;
            for (int j = 0; j < 3; j++) col[j] = col[j] * lit;
        }
        *cov = pn_composite_hit(col, t_hit, t_max, acc, s, d0, out);
    }
    *t_out = t_hit;
}

// SHADOWED: pn_draw_colliders_shadowed's kernel; without it the code below is k_draw_colliders as it has always been, operation for operation.
template <bool SHADOWED>
__device__ __forceinline__ void pn_draw_ray(const pn_contact_state* __restrict__ st, const pn_collider_style& style, const float* __restrict__ rays_o,
                                            const float* __restrict__ rays_d, uint32_t N, float t_min, float t_max, float bg,
                                            const float* __restrict__ weights_sum, const float* __restrict__ depth_0, float* __restrict__ image,
                                            float* __restrict__ coverage, float* __restrict__ collider_t, const pn_shadow_light& lt,
                                            const float* __restrict__ shadow_ws, const float* __restrict__ shadow_depth_0, float* __restrict__ shadow_out) {
    __shared__ PnDrawSlot s_slot[PN_CONTACT_SLOTS];
    __shared__ int s_n, s_new;
    const int tid = threadIdx.x;
    pn_load_slot(st, style, tid, s_slot, &s_n, &s_new);
    __syncthreads();
    const uint32_t i = blockIdx.x * PN_COLLIDER_THREADS + tid;
    if (i >= N) return;
    const size_t i3 = (size_t)i * 3;
    const float o[3] = {rays_o[i3], rays_o[i3 + 1], rays_o[i3 + 2]};
    const float d[3] = {rays_d[i3], rays_d[i3 + 1], rays_d[i3 + 2]};
    const float s = weights_sum[i], d0 = depth_0[i];
    const float acc[3] = {image[i3], image[i3 + 1], image[i3 + 2]};
    const float q = pn_dot3(d, d);
    const int n_slots = s_n;
    const int any_new = s_new;   // the same for every ray of the launch: a scalar branch, and a frame of planes and spheres runs the code it always ran
    float t_hit, out[3] = {acc[0], acc[1], acc[2]}, cov = s, occ = 0.0f;
    if (__builtin_amdgcn_readfirstlane(any_new))
        pn_trace_ray<SHADOWED, true>(s_slot, n_slots, style, o, d, q, t_min, t_max, acc, s, d0, lt, shadow_ws, shadow_depth_0, out, &cov, &occ, &t_hit);
    else
        pn_trace_ray<SHADOWED, false>(s_slot, n_slots, style, o, d, q, t_min, t_max, acc, s, d0, lt, shadow_ws, shadow_depth_0, out, &cov, &occ, &t_hit);
    const float kbg = (1.0f - cov) * bg;
    image[i3] = out[0] + kbg; image[i3 + 1] = out[1] + kbg; image[i3 + 2] = out[2] + kbg;
    if (coverage) coverage[i] = cov;
    if (collider_t) collider_t[i] = t_hit;
    if (SHADOWED && shadow_out) shadow_out[i] = occ;
}

__global__ void __launch_bounds__(PN_COLLIDER_THREADS) k_draw_colliders(const pn_contact_state* __restrict__ st, pn_collider_style style,
                                                                        const float* __restrict__ rays_o, const float* __restrict__ rays_d, uint32_t N,
                                                                        float t_min, float t_max, float bg, const float* __restrict__ weights_sum,
                                                                        const float* __restrict__ depth_0, float* __restrict__ image,
                                                                        float* __restrict__ coverage, float* __restrict__ collider_t) {
    pn_draw_ray<false>(st, style, rays_o, rays_d, N, t_min, t_max, bg, weights_sum, depth_0, image, coverage, collider_t, pn_shadow_light{}, nullptr,
                       nullptr, nullptr);
}

__global__ void __launch_bounds__(PN_COLLIDER_THREADS) k_draw_colliders_shadowed(const pn_contact_state* __restrict__ st, pn_collider_style style,
                                                                                 const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                                                                                 uint32_t N, float t_min, float t_max, float bg,
                                                                                 const float* __restrict__ weights_sum, const float* __restrict__ depth_0,
                                                                                 float* __restrict__ image, float* __restrict__ coverage,
                                                                                 float* __restrict__ collider_t, pn_shadow_light lt,
                                                                                 const float* __restrict__ shadow_ws,
                                                                                 const float* __restrict__ shadow_depth_0, float* __restrict__ shadow_out) {
    pn_draw_ray<true>(st, style, rays_o, rays_d, N, t_min, t_max, bg, weights_sum, depth_0, image, coverage, collider_t, lt, shadow_ws, shadow_depth_0,
                      shadow_out);
}

static bool pn_overlaps(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a && b && a0 < b0 + nb && b0 < a0 + na;
}

// The argument checks both entry points share, up to and including the N == 0 exit: *launch says whether anything is left to do.
static int pn_draw_colliders_scalars(const pn_collider_style* style, uint32_t N, float t_min, float t_max, float bg_scalar, bool* launch) {
    *launch = false;
    PN_REQUIRE(style != nullptr);
    PN_REQUIRE(isfinite(t_min) && isfinite(t_max) && isfinite(bg_scalar) && t_max > t_min);
    for (int k = 0; k < PN_CONTACT_SLOTS; k++)
        for (int j = 0; j < 3; j++) PN_REQUIRE(isfinite(style->rgb[k][j]));
    PN_REQUIRE(isfinite(style->checker) && isfinite(style->checker_dim) && style->ambient >= 0.0f && style->ambient <= 1.0f);
    PN_REQUIRE(N <= 2147483647u / 3u);
    *launch = N != 0;
    return PN_OK;
}

// ... and the pointers: n_in inputs, n_out outputs (a NULL output is absent); no output may overlap an input or another output.
static int pn_draw_colliders_buffers(const void* const* in, const size_t* in_bytes, int n_in, void* const* outp, const size_t* out_bytes, int n_out) {
    for (int a = 0; a < n_out; a++) {
        for (int b = 0; b < n_in; b++) PN_REQUIRE(!pn_overlaps(outp[a], out_bytes[a], in[b], in_bytes[b]));   // an output aliasing an input
        for (int b = a + 1; b < n_out; b++) PN_REQUIRE(!pn_overlaps(outp[a], out_bytes[a], outp[b], out_bytes[b]));
    }
    return PN_OK;
}

extern "C" int pn_draw_colliders(const void* contact_state, const pn_collider_style* style, const float* rays_o, const float* rays_d, uint32_t N,
                                 float t_min, float t_max, float bg_scalar, const float* weights_sum, const float* depth_0, float* image,
                                 float* coverage_out, float* collider_t_out, void* stream) {
    bool launch;
    if (const int rc = pn_draw_colliders_scalars(style, N, t_min, t_max, bg_scalar, &launch)) return rc;
    if (!launch) return PN_OK;
    PN_REQUIRE(contact_state && rays_o && rays_d && weights_sum && depth_0 && image);
    const size_t n1 = (size_t)N * sizeof(float), n3 = 3 * n1;
    const void* in[5] = {rays_o, rays_d, weights_sum, depth_0, contact_state};
    const size_t in_bytes[5] = {n3, n3, n1, n1, sizeof(pn_contact_state)};
    void* outp[3] = {image, coverage_out, collider_t_out};
    const size_t out_bytes[3] = {n3, n1, n1};
    if (const int rc = pn_draw_colliders_buffers(in, in_bytes, 5, outp, out_bytes, 3)) return rc;
    k_draw_colliders<<<pn_div_up(N, PN_COLLIDER_THREADS), PN_COLLIDER_THREADS, 0, (hipStream_t)stream>>>(
        (const pn_contact_state*)contact_state, *style, rays_o, rays_d, N, t_min, t_max, bg_scalar, weights_sum, depth_0, image, coverage_out, collider_t_out);
    PN_LAUNCH_CHECK();
    return PN_OK;
}

extern "C" int pn_draw_colliders_shadowed(const void* contact_state, const pn_collider_style* style, const float* rays_o, const float* rays_d, uint32_t N,
                                          float t_min, float t_max, float bg_scalar, const float* weights_sum, const float* depth_0, float* image,
                                          float* coverage_out, float* collider_t_out, pn_shadow_light light, const float* shadow_ws,
                                          const float* shadow_depth_0, float* shadow_out, void* stream) {
    bool launch;
    if (const int rc = pn_draw_colliders_scalars(style, N, t_min, t_max, bg_scalar, &launch)) return rc;
    PN_REQUIRE(light.S >= 2 && light.S <= 4096);
    for (int j = 0; j < 3; j++) PN_REQUIRE(isfinite(light.c[j]) && isfinite(light.L[j]) && isfinite(light.U[j]) && isfinite(light.V[j]));
    PN_REQUIRE(isfinite(light.half) && isfinite(light.D) && isfinite(light.bias) && light.half > 0.0f);
    PN_REQUIRE(light.strength >= 0.0f && light.strength <= 1.0f);
    if (!launch) return PN_OK;
    PN_REQUIRE(contact_state && rays_o && rays_d && weights_sum && depth_0 && image && shadow_ws && shadow_depth_0);
    const size_t n1 = (size_t)N * sizeof(float), n3 = 3 * n1, nm = (size_t)light.S * (size_t)light.S * sizeof(float);
    const void* in[7] = {rays_o, rays_d, weights_sum, depth_0, contact_state, shadow_ws, shadow_depth_0};
    const size_t in_bytes[7] = {n3, n3, n1, n1, sizeof(pn_contact_state), nm, nm};
    void* outp[4] = {image, coverage_out, collider_t_out, shadow_out};
    const size_t out_bytes[4] = {n3, n1, n1, n1};
    if (const int rc = pn_draw_colliders_buffers(in, in_bytes, 7, outp, out_bytes, 4)) return rc;
    k_draw_colliders_shadowed<<<pn_div_up(N, PN_COLLIDER_THREADS), PN_COLLIDER_THREADS, 0, (hipStream_t)stream>>>(
        (const pn_contact_state*)contact_state, *style, rays_o, rays_d, N, t_min, t_max, bg_scalar, weights_sum, depth_0, image, coverage_out, collider_t_out,
        light, shadow_ws, shadow_depth_0, shadow_out);
    PN_LAUNCH_CHECK();
    return PN_OK;
}
