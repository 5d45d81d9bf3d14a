// The GUI's mouse drag on the device (nerf/gui.py:556-586 per frame, :833-841 pick, :647-657 screen_to_world of the reference).
//
// The GUI reads the picked integration point's position back to the host every frame and hands the simulator a spring force toward the cursor.
// Here the force is computed by a kernel enqueued in front of every substep (k_drag_force) from a small state in device memory (pn_drag_state:
// picked IP, cursor target, force scale), so a substep captured into a HIP graph — or run frames ahead of the render in the pipelined harness —
// gets the spring force of ITS OWN state; the host only writes the target (k_drag_unproject, per cursor move) and reads the picked IP once per
// click.
#include <math.h>

#include "pn_common.h"
#include "pn_sim_ip.h"

static_assert(sizeof(pn_drag_state) == 40, "pn_drag_state: 40 bytes (pienerf_amd/simulator/drag.py allocates it as 5 doubles)");

#define PN_DRAG_BLOCKS 128       // workgroups of the zero-depth fallback's first pass (fixed: the sum's order must not depend on the device)
#define PN_DRAG_THREADS 256
#define PN_DRAG_PICK_THREADS 1024

struct PnDragCam {
    double x, y, fx, fy, cx, cy;
    double pose[16];  // c2w, row-major, the caller's fp32 values widened
};

// ------------------------------------------------------------------------------------------------ the spring force, every substep
// gui.py:556-586: p0 = get_IP_info()[0][vid] (fp32), f = scale * 1e5 * (target - p0) in fp64, |f| clamped to 5e5, then update_force(vid, f).
// Every workgroup computes the same f (one lane; a serial sum, to have get_IP_info's bits) and writes its share of dof_f with update_force's formula.
// active == 0: dof_f = 0 (clear_force).
__global__ void __launch_bounds__(PN_DRAG_THREADS) k_drag_force(int n30, int n_IP, const pn_drag_state* __restrict__ drag, const double* __restrict__ dof,
                                                                double dx3, const int* __restrict__ topo, const double* __restrict__ rho,
                                                                const double* __restrict__ Nx, double* __restrict__ dof_f) {
    __shared__ int s_kid[8];
    __shared__ double s_N[80], s_d[240], s_f[3];
    const int t = threadIdx.x;
    const int vid = drag->vid;
    const bool on = drag->active != 0 && vid >= 0 && vid < n_IP;  // uniform over the workgroup
    if (on) {
        if (t < 8) s_kid[t] = topo[vid * 8 + t];
        if (t < 80) s_N[t] = Nx[(size_t)vid * 80 + t];
        __syncthreads();
        if (t < 240) s_d[t] = dof[(size_t)s_kid[t / 30] * 30 + t % 30];
        __syncthreads();
        if (t == 0) {
            double a0 = 0, a1 = 0, a2 = 0;
            for (int i = 0; i < 8; i++) pn_ip_row_acc(s_d + i * 30, s_N + i * 10, a0, a1, a2);  // k_update_F's row 0
            const double p0[3] = {(double)(float)a0, (double)(float)a1, (double)(float)a2};
            const double k = drag->scale * 1e5;
            double f[3];
            for (int c = 0; c < 3; c++) f[c] = k * (drag->target[c] - p0[c]);
            const double n = sqrt(__dadd_rn(__dadd_rn(__dmul_rn(f[0], f[0]), __dmul_rn(f[1], f[1])), __dmul_rn(f[2], f[2])));
            if (n > 5e5) {
                const double c = 5e5 / n;
                for (int i = 0; i < 3; i++) f[i] *= c;
            }
            s_f[0] = f[0]; s_f[1] = f[1]; s_f[2] = f[2];
        }
        __syncthreads();
    }
    const int o = t + blockIdx.x * blockDim.x;
    if (o >= n30) return;
    dof_f[o] = on ? pn_force_entry(o, vid, s_f[0], s_f[1], s_f[2], dx3, topo, rho, Nx) : 0.0;
}

extern "C" uint64_t pn_sim_drag_bytes(void) { return sizeof(pn_drag_state); }
extern "C" uint64_t pn_sim_drag_work_doubles(void) { return 2 * PN_DRAG_BLOCKS; }

extern "C" int pn_sim_drag_force(int n_k, int n_IP, const void* drag, const double* dof, double dx, const int* topo, const double* rho, const double* Nx,
                                 double* dof_f, void* stream) {
    PN_REQUIRE(n_k > 0 && n_IP > 0 && drag && dof && topo && rho && Nx && dof_f);
    k_drag_force<<<pn_div_up((uint64_t)n_k * 30, PN_DRAG_THREADS), PN_DRAG_THREADS, 0, (hipStream_t)stream>>>(
        n_k * 30, n_IP, (const pn_drag_state*)drag, dof, pow(dx, 3.0), topo, rho, Nx, dof_f);
    PN_LAUNCH_CHECK();
    return PN_OK;
}

// ------------------------------------------------------------------------------------------------ host-side updates
__global__ void k_drag_set(pn_drag_state* __restrict__ drag, int vid, int active, double scale, int set_target, double tx, double ty, double tz) {
    if (vid >= 0) drag->vid = vid;
    if (active >= 0) drag->active = active;
    if (scale > 0.0) drag->scale = scale;
    if (set_target) {
        drag->target[0] = tx; drag->target[1] = ty; drag->target[2] = tz;
    }
}

extern "C" int pn_sim_drag_set(void* drag, int n_IP, int vid, int active, double scale, const double* target3_host, void* stream) {
    PN_REQUIRE(drag && n_IP > 0 && vid < n_IP && active <= 1 && isfinite(scale));
    const double* t = target3_host;
    PN_REQUIRE(!t || (isfinite(t[0]) && isfinite(t[1]) && isfinite(t[2])));
    k_drag_set<<<1, 1, 0, (hipStream_t)stream>>>((pn_drag_state*)drag, vid, active, scale, t != nullptr, t ? t[0] : 0.0, t ? t[1] : 0.0, t ? t[2] : 0.0);
    PN_LAUNCH_CHECK();
    return PN_OK;
}

// ------------------------------------------------------------------------------------------------ screen_to_world (+ pick)
// Zero depth under the cursor: the reference falls back to np.mean(depth[np.nonzero(depth)]).  First pass: PN_DRAG_BLOCKS workgroups, each the fp64
// sum and count of the nonzero entries of a fixed strided share, reduced in a fixed tree (wave shuffles, then the waves in order) — the same bits on
// every run.  Nothing is done when the depth under the cursor is nonzero.
__device__ __forceinline__ void pn_drag_wave_sum2(double& s, double& c) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s += __shfl_down(s, off);
        c += __shfl_down(c, off);
    }
}

__global__ void __launch_bounds__(PN_DRAG_THREADS) k_drag_depth_partial(const float* __restrict__ depth, int n, int pix, double* __restrict__ work) {
    __shared__ double s_s[PN_DRAG_THREADS / 64], s_c[PN_DRAG_THREADS / 64];
    if (depth[pix] != 0.0f) return;  // uniform
    double s = 0.0, c = 0.0;
    for (int i = blockIdx.x * PN_DRAG_THREADS + threadIdx.x; i < n; i += PN_DRAG_BLOCKS * PN_DRAG_THREADS) {
        const float d = depth[i];
        if (d != 0.0f) {  // np.nonzero: NaN counts as nonzero, as there
            s += (double)d;
            c += 1.0;
        }
    }
    pn_drag_wave_sum2(s, c);
    const int w = threadIdx.x / 64, lane = threadIdx.x % 64;
    if (lane == 0) { s_s[w] = s; s_c[w] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < PN_DRAG_THREADS / 64; i++) { s += s_s[i]; c += s_c[i]; }
        work[blockIdx.x * 2] = s;
        work[blockIdx.x * 2 + 1] = c;
    }
}

// One workgroup.  Lane 0: the depth under the cursor (or the fallback mean, rounded to fp32 as numpy's mean of an fp32 array is), the camera
// point ((x-cx)/fx d, (y-cy)/fy d, d) and pose @ [xs, ys, zs, 1] in fp64, summed left to right without contraction (numpy's order for the
// host restatement).  n_IP > 0 (a click): vid = argmin over the IPs of |p - target|^2 ((dx^2 + dy^2) + dz^2, fp64 from the fp32 positions), the
// lowest index on ties (np.argmin): every lane keeps the first minimum of its ascending strided share, then a fixed tree over lanes and waves
// that prefers the lower index on equal distances.  An all-zero depth image leaves the target as it was (numpy would give NaN).
__global__ void __launch_bounds__(PN_DRAG_PICK_THREADS) k_drag_unproject(const float* __restrict__ depth, int pix, PnDragCam cam,
                                                                        const double* __restrict__ work, const float* __restrict__ ip_pos, int n_IP,
                                                                        pn_drag_state* __restrict__ drag) {
    __shared__ double s_t[3];
    __shared__ double s_bd[PN_DRAG_PICK_THREADS / 64];
    __shared__ int s_bi[PN_DRAG_PICK_THREADS / 64];
    const int t = threadIdx.x;
    if (t == 0) {
        double d = (double)depth[pix];
        bool ok = true;
        if (d == 0.0) {
            double s = 0.0, c = 0.0;
            for (int b = 0; b < PN_DRAG_BLOCKS; b++) { s += work[b * 2]; c += work[b * 2 + 1]; }
            ok = c > 0.0;
            d = (double)(float)(s / c);
        }
        if (ok) {
            const double xs = (cam.x - cam.cx) / cam.fx * d, ys = (cam.y - cam.cy) / cam.fy * d, zs = d;
            for (int r = 0; r < 3; r++) {
                const double* P = cam.pose + r * 4;
                const double p = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(P[0], xs), __dmul_rn(P[1], ys)), __dmul_rn(P[2], zs)), P[3]);
                drag->target[r] = p;
            }
        }
        s_t[0] = drag->target[0]; s_t[1] = drag->target[1]; s_t[2] = drag->target[2];
    }
    if (n_IP <= 0) return;  // uniform: target only
    __syncthreads();
    const double tx = s_t[0], ty = s_t[1], tz = s_t[2];
    double bd = INFINITY;
    int bi = 0x7fffffff;
    for (int i = t; i < n_IP; i += PN_DRAG_PICK_THREADS) {
        const double dx = (double)ip_pos[i * 3] - tx, dy = (double)ip_pos[i * 3 + 1] - ty, dz = (double)ip_pos[i * 3 + 2] - tz;
        const double q = __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
        if (q < bd) { bd = q; bi = i; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double od = __shfl_down(bd, off);
        const int oi = __shfl_down(bi, off);
        if (od < bd || (od == bd && oi < bi)) { bd = od; bi = oi; }
    }
    const int w = t / 64, lane = t % 64;
    if (lane == 0) { s_bd[w] = bd; s_bi[w] = bi; }
    __syncthreads();
    if (t == 0) {
        for (int i = 1; i < PN_DRAG_PICK_THREADS / 64; i++)
            if (s_bd[i] < bd || (s_bd[i] == bd && s_bi[i] < bi)) { bd = s_bd[i]; bi = s_bi[i]; }
        drag->vid = bi < n_IP ? bi : 0;  // every distance NaN: np.argmin answers 0
        drag->active = 1;
    }
}

extern "C" int pn_sim_drag_unproject(const float* depth0, int W, int H, double x, double y, const double* intr4, const double* pose16, const float* ip_pos,
                                     int n_IP, void* drag, double* work, void* stream) {
    PN_REQUIRE(depth0 && W > 0 && H > 0 && intr4 && pose16 && drag && work && n_IP >= 0 && (n_IP == 0 || ip_pos));
    PN_REQUIRE(isfinite(intr4[0]) && isfinite(intr4[1]) && intr4[0] != 0.0 && intr4[1] != 0.0 && isfinite(intr4[2]) && isfinite(intr4[3]));
    PN_REQUIRE(intr4[2] >= 0.0 && intr4[3] >= 0.0 && intr4[2] < 1e9 && intr4[3] < 1e9);
    for (int i = 0; i < 16; i++) PN_REQUIRE(isfinite(pose16[i]));
    // the reference reads depth.reshape(2 int(cx), 2 int(cy))[int(x), int(y)]: the image must have that many pixels, the pixel must lie inside
    const int64_t rx = 2 * (int64_t)intr4[2], ry = 2 * (int64_t)intr4[3];
    PN_REQUIRE(rx * ry == (int64_t)W * H);
    PN_REQUIRE(isfinite(x) && isfinite(y) && x >= 0.0 && y >= 0.0 && x < (double)rx && y < (double)ry);
    const int pix = (int)((int64_t)x * ry + (int64_t)y);
    PnDragCam cam;
    cam.x = x; cam.y = y; cam.fx = intr4[0]; cam.fy = intr4[1]; cam.cx = intr4[2]; cam.cy = intr4[3];
    for (int i = 0; i < 16; i++) cam.pose[i] = pose16[i];
    hipStream_t s = (hipStream_t)stream;
    k_drag_depth_partial<<<PN_DRAG_BLOCKS, PN_DRAG_THREADS, 0, s>>>(depth0, W * H, pix, work);
    PN_LAUNCH_CHECK();
    k_drag_unproject<<<1, PN_DRAG_PICK_THREADS, 0, s>>>(depth0, pix, cam, work, ip_pos, n_IP, (pn_drag_state*)drag);
    PN_LAUNCH_CHECK();
    return PN_OK;
}
