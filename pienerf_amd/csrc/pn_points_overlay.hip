// The simulator's integration points and the drag handle drawn into a rendered frame (include/pienerf_hip.h: pn_draw_points has the law).
//
// Two launches behind the frame driver, the colliders' launch and the background's blend: k_points_splat, a thread per point, projects the point and
// takes an unsigned 64-bit atomic min of (bits(t) << 32 | index) on every pixel of its footprint; k_points_resolve, a thread per pixel, reads the key,
// writes the empty value back (the buffer cleans itself: no memset per frame), depth-tests the winner against the object and the colliders, colours it,
// blends it into `image` and then evaluates the drag handle's two discs and its line.  The min makes the result a function of the points alone: the
// nearest point per pixel, the lowest index on ties, in whatever order the hardware ran the threads.  Positions, F, the pose and the drag state are read
// on the device: a launch captured into a HIP graph follows the simulator, the camera and the cursor.  Built with -ffp-contract=off: every operation
// rounds once, in the order written here, which tests/points_overlay_reference.py restates in numpy.
#include <math.h>

#include "pn_common.h"

static_assert(sizeof(pn_point_style) == 88, "pn_point_style: 22 four-byte members (pienerf_amd/_lib.py: PointStyle)");
static_assert(sizeof(pn_drag_state) == 40, "pn_drag_state: vid, active, target[3], scale");

#define PN_POINTS_THREADS 256
#define PN_POINTS_EMPTY 0xffffffffffffffffull

struct PnCamera {
    float R[9], c[3];          // c2w rotation, row-major, and the camera's centre
    float fx, fy, cx, cy;
};

__device__ __forceinline__ PnCamera pn_load_camera(const float* __restrict__ pose16, float fx, float fy, float cx, float cy) {
    PnCamera cam;
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) cam.R[r * 3 + c] = pose16[r * 4 + c];
        cam.c[r] = pose16[r * 4 + 3];
    }
    cam.fx = fx; cam.fy = fy; cam.cx = cx; cam.cy = cy;
    return cam;
}

// Camera coordinates xc = R^T (x - c), the distance t = |x - c| and the screen position (u, v) = (xc / zc fx + cx, yc / zc fy + cy).  Returns whether
// the point can be drawn at all: finite coordinates and in front of the camera (zc > 0).
__device__ __forceinline__ bool pn_project(const PnCamera& cam, const float x[3], float* u, float* v, float* t) {
    const float d0 = x[0] - cam.c[0], d1 = x[1] - cam.c[1], d2 = x[2] - cam.c[2];
    const float xc = cam.R[0] * d0 + cam.R[3] * d1 + cam.R[6] * d2;
    const float yc = cam.R[1] * d0 + cam.R[4] * d1 + cam.R[7] * d2;
    const float zc = cam.R[2] * d0 + cam.R[5] * d1 + cam.R[8] * d2;
    *t = sqrtf(d0 * d0 + d1 * d1 + d2 * d2);
    *u = xc / zc * cam.fx + cam.cx;
    *v = yc / zc * cam.fy + cam.cy;
    return isfinite(x[0]) && isfinite(x[1]) && isfinite(x[2]) && zc > 0.0f && isfinite(*t) && isfinite(*u) && isfinite(*v);
}

__global__ void __launch_bounds__(PN_POINTS_THREADS) k_points_splat(const float* __restrict__ pos, int n, const float* __restrict__ pose16, float fx, float fy,
                                                                    float cx, float cy, int W, int H, float t_min, int radius,
                                                                    unsigned long long* keys) {
    const unsigned iu = blockIdx.x * (unsigned)PN_POINTS_THREADS + threadIdx.x;   // unsigned: n may be close to 2^31
    if (iu >= (unsigned)n) return;
    const int i = (int)iu;
    const PnCamera cam = pn_load_camera(pose16, fx, fy, cx, cy);
    const float x[3] = {pos[(size_t)i * 3], pos[(size_t)i * 3 + 1], pos[(size_t)i * 3 + 2]};
    float u, v, t;
    if (!pn_project(cam, x, &u, &v, &t) || !(t > t_min)) return;
    const float fpx = floorf(u), fpy = floorf(v);
    // range-checked in float before the conversion: a footprint of radius <= 8 around a pixel outside this band holds no pixel of the image
    if (!(fpx >= -9.0f && fpx <= (float)W + 8.0f && fpy >= -9.0f && fpy <= (float)H + 8.0f)) return;
    const int px = (int)fpx, py = (int)fpy;
    const unsigned long long key = ((unsigned long long)__float_as_uint(t) << 32) | (unsigned)i;   // t > 0: its bits order as the floats do
    const int r2 = radius * radius;
    for (int dy = -radius; dy <= radius; dy++) {
        const int y = py + dy;
        if (y < 0 || y >= H) continue;
        for (int dx = -radius; dx <= radius; dx++) {
            const int xx = px + dx;
            if (xx < 0 || xx >= W || dx * dx + dy * dy > r2) continue;
            unsigned long long* k = keys + ((size_t)y * W + xx);
            // min is monotone: a stored key already below ours cannot be changed by it, whatever happens to the pixel meanwhile
            if (*(volatile unsigned long long*)k <= key) continue;
            __hip_atomic_fetch_min(k, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// The ramp modes' scalar of point i (include/pienerf_hip.h: pn_draw_points has the formulas).
__device__ __forceinline__ float pn_point_scalar(int mode, const float* __restrict__ F, const float* __restrict__ values, int i) {
    if (mode == PN_POINT_VALUES) return values[i];
    float f[9];
    for (int k = 0; k < 9; k++) f[k] = F[(size_t)i * 9 + k];
    if (mode == PN_POINT_VOLUME) {
        const float det = f[0] * (f[4] * f[8] - f[5] * f[7]) - f[1] * (f[3] * f[8] - f[5] * f[6]) + f[2] * (f[3] * f[7] - f[4] * f[6]);
        return det - 1.0f;
    }
    float sum = 0.0f;
    for (int a = 0; a < 3; a++) {
        for (int b = 0; b < 3; b++) {
            const float C = f[a] * f[b] + f[3 + a] * f[3 + b] + f[6 + a] * f[6 + b];
            const float E = 0.5f * (C - (a == b ? 1.0f : 0.0f));
            sum = sum + E * E;
        }
    }
    return sqrtf(sum);
}

// The drag handle as the pixels read it, once per workgroup.
struct PnMarkers {
    int a_ok, b_ok;            // the picked point / the target can be drawn
    float ax, ay, bx, by;
};

__global__ void __launch_bounds__(PN_POINTS_THREADS) k_points_resolve(const float* __restrict__ pos, const float* __restrict__ F,
                                                                      const float* __restrict__ values, int n, const float* __restrict__ pose16, float fx,
                                                                      float fy, float cx, float cy, int W, int N, const float* __restrict__ weights_sum,
                                                                      const float* __restrict__ depth_0, const float* __restrict__ collider_t,
                                                                      const pn_drag_state* __restrict__ drag, unsigned long long* keys, pn_point_style st,
                                                                      float* image, int* __restrict__ point_id, float* __restrict__ point_t) {
    __shared__ PnMarkers s_m;
    if (threadIdx.x == 0) {
        PnMarkers m;
        m.a_ok = m.b_ok = 0;
        m.ax = m.ay = m.bx = m.by = 0.0f;
        if (drag != nullptr && drag->active != 0) {
            const PnCamera cam = pn_load_camera(pose16, fx, fy, cx, cy);
            const int vid = drag->vid;
            float t;
            if (vid >= 0 && vid < n) {
                const float x[3] = {pos[(size_t)vid * 3], pos[(size_t)vid * 3 + 1], pos[(size_t)vid * 3 + 2]};
                m.a_ok = pn_project(cam, x, &m.ax, &m.ay, &t) ? 1 : 0;
            }
            const float y[3] = {(float)drag->target[0], (float)drag->target[1], (float)drag->target[2]};
            m.b_ok = pn_project(cam, y, &m.bx, &m.by, &t) ? 1 : 0;
        }
        s_m = m;
    }
    __syncthreads();
    const unsigned pu = blockIdx.x * (unsigned)PN_POINTS_THREADS + threadIdx.x;   // unsigned: N may be close to 2^31
    if (pu >= (unsigned)N) return;
    const int p = (int)pu;
    const unsigned long long key = keys[p];
    if (key != PN_POINTS_EMPTY) keys[p] = PN_POINTS_EMPTY;
    const size_t p3 = (size_t)p * 3;
    float out[3];
    bool changed = false, loaded = false;
    int id = -1;
    float t_id = INFINITY;
    const unsigned idx = (unsigned)(key & 0xffffffffull);
    if (key != PN_POINTS_EMPTY && idx < (unsigned)n) {
        const int i = (int)idx;
        const float t = __uint_as_float((unsigned)(key >> 32));
        const float s = weights_sum[p];
        const float t_obj = s > 1e-4f ? depth_0[p] / s : INFINITY;
        const float t_front = collider_t != nullptr ? fminf(t_obj, collider_t[p]) : t_obj;
        const bool visible = st.xray != 0 || t <= t_front + st.bias;
        if (visible || st.hidden_alpha != 0.0f) {
            const float a = visible ? st.alpha : st.alpha * st.hidden_alpha;
            float c[3];
            if (st.mode == PN_POINT_FLAT) {
                c[0] = st.rgb[0]; c[1] = st.rgb[1]; c[2] = st.rgb[2];
            } else {
                const float v = pn_point_scalar(st.mode, F, values, i);
                const float u = fminf(fmaxf((v - st.lo) / (st.hi - st.lo), 0.0f), 1.0f);
                const bool low = u < 0.5f;
                const float w = low ? u * 2.0f : (u - 0.5f) * 2.0f;
                for (int j = 0; j < 3; j++) {
                    const float r0 = low ? st.ramp[0][j] : st.ramp[1][j], r1 = low ? st.ramp[1][j] : st.ramp[2][j];
                    c[j] = r0 + w * (r1 - r0);
                }
            }
            for (int j = 0; j < 3; j++) out[j] = a * c[j] + (1.0f - a) * image[p3 + j];
            changed = loaded = true;
            id = i;
            t_id = t;
        }
    }
    const PnMarkers m = s_m;
    if (m.a_ok || m.b_ok) {
        const float qx = (float)(p % W) + 0.5f, qy = (float)(p / W) + 0.5f;
        const float rr = st.marker_radius * st.marker_radius;
        if (m.a_ok) {
            const float dx = qx - m.ax, dy = qy - m.ay;
            if (dx * dx + dy * dy <= rr) { out[0] = 1.0f; out[1] = 0.0f; out[2] = 0.0f; changed = loaded = true; }
        }
        if (m.b_ok) {
            const float dx = qx - m.bx, dy = qy - m.by;
            if (dx * dx + dy * dy <= rr) { out[0] = 0.0f; out[1] = 0.0f; out[2] = 1.0f; changed = loaded = true; }
        }
        if (m.a_ok && m.b_ok) {
            const float ex = m.bx - m.ax, ey = m.by - m.ay;
            const float dx = qx - m.ax, dy = qy - m.ay;
            const float L2 = ex * ex + ey * ey;
            const float h = L2 > 0.0f ? fminf(fmaxf((dx * ex + dy * ey) / L2, 0.0f), 1.0f) : 0.0f;
            const float gx = dx - h * ex, gy = dy - h * ey;
            const float half = 0.5f * st.marker_thickness;
            if (gx * gx + gy * gy <= half * half) {
                if (!loaded) { out[0] = image[p3]; out[1] = image[p3 + 1]; out[2] = image[p3 + 2]; }
                const float keep = 1.0f - 100.0f / 255.0f;
                for (int j = 0; j < 3; j++) out[j] = keep * out[j];
                changed = true;
            }
        }
    }
    if (changed) { image[p3] = out[0]; image[p3 + 1] = out[1]; image[p3 + 2] = out[2]; }
    if (point_id) point_id[p] = id;
    if (point_t) point_t[p] = t_id;
}

static bool pn_points_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a && b && a0 < b0 + nb && b0 < a0 + na;
}

extern "C" uint64_t pn_points_keys_bytes(int W, int H) {
    if (W <= 0 || H <= 0) return 0;
    return (uint64_t)W * (uint64_t)H * sizeof(uint64_t);
}

extern "C" int pn_draw_points(const float* pos, const float* F, const float* values, int64_t n, const float* pose16, const float* intr4_host, int W, int H,
                              float t_min, const float* weights_sum, const float* depth_0, const float* collider_t, const void* drag, uint64_t* keys,
                              pn_point_style style, float* image, int* point_id_out, float* point_t_out, void* stream) {
    PN_REQUIRE(n >= 0 && n <= 2147483647ll && W > 0 && H > 0 && (int64_t)W * (int64_t)H <= 2147483647ll);
    PN_REQUIRE(intr4_host != nullptr && isfinite(t_min));
    const float fx = intr4_host[0], fy = intr4_host[1], cx = intr4_host[2], cy = intr4_host[3];
    PN_REQUIRE(isfinite(fx) && isfinite(fy) && isfinite(cx) && isfinite(cy));
    PN_REQUIRE(style.radius >= 0 && style.radius <= 8);
    PN_REQUIRE(style.mode >= PN_POINT_FLAT && style.mode <= PN_POINT_VALUES);
    for (int j = 0; j < 3; j++) {
        PN_REQUIRE(isfinite(style.rgb[j]));
        for (int k = 0; k < 3; k++) PN_REQUIRE(isfinite(style.ramp[k][j]));
    }
    PN_REQUIRE(isfinite(style.lo) && isfinite(style.hi) && isfinite(style.bias) && isfinite(style.marker_radius) && isfinite(style.marker_thickness));
    PN_REQUIRE(style.alpha >= 0.0f && style.alpha <= 1.0f && style.hidden_alpha >= 0.0f && style.hidden_alpha <= 1.0f);
    if (style.mode != PN_POINT_FLAT) PN_REQUIRE(style.hi > style.lo);
    if (style.mode == PN_POINT_STRAIN || style.mode == PN_POINT_VOLUME) PN_REQUIRE(F != nullptr);
    if (style.mode == PN_POINT_VALUES) PN_REQUIRE(values != nullptr);
    if (n == 0 && drag == nullptr) return PN_OK;   // nothing to draw: nothing launched
    PN_REQUIRE(pose16 && weights_sum && depth_0 && keys && image && (n == 0 || pos));
    const size_t N = (size_t)W * (size_t)H, n1 = N * sizeof(float), nn = (size_t)n * sizeof(float);
    const void* in[8] = {pos, F, values, pose16, weights_sum, depth_0, collider_t, drag};
    const size_t in_bytes[8] = {3 * nn, 9 * nn, nn, 16 * sizeof(float), n1, n1, n1, sizeof(pn_drag_state)};
    void* outp[4] = {image, point_id_out, point_t_out, keys};
    const size_t out_bytes[4] = {3 * n1, n1, n1, N * sizeof(uint64_t)};
    for (int a = 0; a < 4; a++) {
        for (int b = 0; b < 8; b++) PN_REQUIRE(!pn_points_overlap(outp[a], out_bytes[a], in[b], in_bytes[b]));   // an output aliasing an input
        for (int b = a + 1; b < 4; b++) PN_REQUIRE(!pn_points_overlap(outp[a], out_bytes[a], outp[b], out_bytes[b]));
    }
    if (n > 0) {
        k_points_splat<<<pn_div_up((uint64_t)n, PN_POINTS_THREADS), PN_POINTS_THREADS, 0, (hipStream_t)stream>>>(
            pos, (int)n, pose16, fx, fy, cx, cy, W, H, t_min, style.radius, (unsigned long long*)keys);
        PN_LAUNCH_CHECK();
    }
    k_points_resolve<<<pn_div_up(N, PN_POINTS_THREADS), PN_POINTS_THREADS, 0, (hipStream_t)stream>>>(
        pos, F, values, (int)n, pose16, fx, fy, cx, cy, W, (int)N, weights_sum, depth_0, collider_t, (const pn_drag_state*)drag, (unsigned long long*)keys,
        style, image, point_id_out, point_t_out);
    PN_LAUNCH_CHECK();
    return PN_OK;
}
