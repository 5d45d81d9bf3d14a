// The contact colliders drawn into a rendered frame (include/pienerf_hip.h: pn_draw_colliders has the law).
//
// The colliders are analytic surfaces in the world space of the rays, and a finished frame carries what a depth-tested composite needs per ray
// (weights_sum, depth_0), so this is one per-ray launch behind the frame driver, as the background model's blend is (pn_background.hip).  The state is
// read on the device: a launch captured into a HIP graph draws the colliders where set_collider last put them.  Built with -ffp-contract=off: every
// operation rounds once, in the order written here, which tests/colliders_reference.py restates in numpy.
#include <math.h>

#include "pn_common.h"

static_assert(sizeof(pn_collider_style) == 108, "pn_collider_style: 27 floats (pienerf_amd/_lib.py: ColliderStyle)");
static_assert(PN_CONTACT_SLOTS == 8, "pn_collider_style.rgb: one colour per collider slot");

#define PN_COLLIDER_THREADS 256

// A slot as the rays read it: the state's fp64 fields rounded to fp32, and a plane's tangent frame, once per workgroup.
struct PnDrawSlot {
    int type;
    float p[3], n[3], R;
    float u[3], v[3];
    float rgb[3];
};

__device__ __forceinline__ float pn_dot3(const float a[3], const float b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

__global__ void __launch_bounds__(PN_COLLIDER_THREADS) k_draw_colliders(const pn_contact_state* __restrict__ st, pn_collider_style style,
                                                                        const float* __restrict__ rays_o, const float* __restrict__ rays_d, uint32_t N,
                                                                        float t_min, float t_max, float bg, const float* __restrict__ weights_sum,
                                                                        const float* __restrict__ depth_0, float* __restrict__ image,
                                                                        float* __restrict__ coverage, float* __restrict__ collider_t) {
    __shared__ PnDrawSlot s_slot[PN_CONTACT_SLOTS];
    __shared__ int s_n;
    const int tid = threadIdx.x;
    if (tid < PN_CONTACT_SLOTS) {
        const pn_contact_collider* c = st->c + tid;
        PnDrawSlot* s = s_slot + tid;
        const int type = c->type;
        s->type = (type >= PN_CONTACT_PLANE && type <= PN_CONTACT_CONTAINER) ? type : PN_CONTACT_EMPTY;
        float n[3];
        for (int i = 0; i < 3; i++) {
            s->p[i] = (float)c->p[i];
            s->n[i] = n[i] = (float)c->n[i];
            s->rgb[i] = style.rgb[tid][i];
        }
        s->R = (float)c->R;
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
        if (tid == 0) s_n = min(max(st->n, 0), PN_CONTACT_SLOTS);
    }
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
    float t_hit = INFINITY;
    int k_hit = -1;
    for (int k = 0; k < n_slots; k++) {   // the slot's type is uniform over the workgroup: no lane diverges on it
        const PnDrawSlot* c = s_slot + k;
        const int type = c->type;
        if (type == PN_CONTACT_EMPTY) continue;
        float t;
        if (type == PN_CONTACT_PLANE) {
            const float nd = pn_dot3(c->n, d);
            if (!(nd < 0.0f)) continue;   // front face only
            const float po[3] = {c->p[0] - o[0], c->p[1] - o[1], c->p[2] - o[2]};
            t = pn_dot3(c->n, po) / nd;
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
        if (t < t_hit) { t_hit = t; k_hit = k; }
    }
    float out[3] = {acc[0], acc[1], acc[2]}, cov = s;
    if (k_hit >= 0) {
        const PnDrawSlot* c = s_slot + k_hit;
        const float t = t_hit;
        const float x[3] = {o[0] + t * d[0], o[1] + t * d[1], o[2] + t * d[2]};
        const float r[3] = {x[0] - c->p[0], x[1] - c->p[1], x[2] - c->p[2]};
        float factor = 1.0f, nd;
        if (c->type == PN_CONTACT_PLANE) {
            nd = pn_dot3(c->n, d);
            if (style.checker > 0.0f) {
                const float cells = floorf(pn_dot3(c->u, r) / style.checker) + floorf(pn_dot3(c->v, r) / style.checker);
                const float half = cells * 0.5f;   // parity without an integer conversion: exact below 2^24 cells, even beyond
                if (half != floorf(half)) factor = style.checker_dim;
            }
        } else {
            const float nrm[3] = {r[0] / c->R, r[1] / c->R, r[2] / c->R};   // the container's sign drops out of |n.d|
            nd = pn_dot3(nrm, d);
        }
        const float shade = style.ambient + (1.0f - style.ambient) * (fabsf(nd) / sqrtf(q));
        const float col[3] = {c->rgb[0] * factor * shade, c->rgb[1] * factor * shade, c->rgb[2] * factor * shade};
        const float a = fminf(fmaxf((t_max - t) / (0.5f * t_max), 0.0f), 1.0f);
        const float t_obj = s > 1e-4f ? d0 / s : INFINITY;
        if (t < t_obj) {   // in front of the object
            for (int j = 0; j < 3; j++) out[j] = a * col[j] + (1.0f - a) * acc[j];
            cov = a + (1.0f - a) * s;
        } else {           // behind it
            const float w = (1.0f - s) * a;
            for (int j = 0; j < 3; j++) out[j] = acc[j] + w * col[j];
            cov = s + w;
        }
    }
    const float kbg = (1.0f - cov) * bg;
    image[i3] = out[0] + kbg; image[i3 + 1] = out[1] + kbg; image[i3 + 2] = out[2] + kbg;
    if (coverage) coverage[i] = cov;
    if (collider_t) collider_t[i] = t_hit;
}

static bool pn_overlaps(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a && b && a0 < b0 + nb && b0 < a0 + na;
}

extern "C" int pn_draw_colliders(const void* contact_state, const pn_collider_style* style, const float* rays_o, const float* rays_d, uint32_t N,
                                 float t_min, float t_max, float bg_scalar, const float* weights_sum, const float* depth_0, float* image,
                                 float* coverage_out, float* collider_t_out, void* stream) {
    PN_REQUIRE(style != nullptr);
    PN_REQUIRE(isfinite(t_min) && isfinite(t_max) && isfinite(bg_scalar) && t_max > t_min);
    for (int k = 0; k < PN_CONTACT_SLOTS; k++)
        for (int j = 0; j < 3; j++) PN_REQUIRE(isfinite(style->rgb[k][j]));
    PN_REQUIRE(isfinite(style->checker) && isfinite(style->checker_dim) && style->ambient >= 0.0f && style->ambient <= 1.0f);
    PN_REQUIRE(N <= 2147483647u / 3u);
    if (N == 0) return PN_OK;
    PN_REQUIRE(contact_state && rays_o && rays_d && weights_sum && depth_0 && image);
    const size_t n1 = (size_t)N * sizeof(float), n3 = 3 * n1;
    const void* in[5] = {rays_o, rays_d, weights_sum, depth_0, contact_state};
    const size_t in_bytes[5] = {n3, n3, n1, n1, sizeof(pn_contact_state)};
    const void* outp[3] = {image, coverage_out, collider_t_out};
    const size_t out_bytes[3] = {n3, n1, n1};
    for (int a = 0; a < 3; a++) {
        for (int b = 0; b < 5; b++) PN_REQUIRE(!pn_overlaps(outp[a], out_bytes[a], in[b], in_bytes[b]));   // an output aliasing an input
        for (int b = a + 1; b < 3; b++) PN_REQUIRE(!pn_overlaps(outp[a], out_bytes[a], outp[b], out_bytes[b]));
    }
    k_draw_colliders<<<pn_div_up(N, PN_COLLIDER_THREADS), PN_COLLIDER_THREADS, 0, (hipStream_t)stream>>>(
        (const pn_contact_state*)contact_state, *style, rays_o, rays_d, N, t_min, t_max, bg_scalar, weights_sum, depth_0, image, coverage_out, collider_t_out);
    PN_LAUNCH_CHECK();
    return PN_OK;
}
