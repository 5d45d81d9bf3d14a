// The t-sequence of a ray (pn_march_window.h, head comment) and one point of it: what the windowed march and the skip pre-pass in front of it
// (pn_march_skip.h) share.  The ray's constants and start, the step and its lattice form, and the pieces of one evaluation that need no candidates —
// each written ONCE, with the argument why it equals the reference bit for bit beside it (-ffp-contract=off: every operation rounds once, in source order).
#pragma once
#include "pn_march_tables.h"

namespace pnm3 {
using namespace pnm;
using pnm2::March2Tables;
using pnm2::warp_record;

struct RayConsts {
    float ox, oy, oz, dx, dy, dz, rdx, rdy, rdz;
    float bmin0, bmin1, bmin2, bmax0, bmax1, bmax2, hi0, hi1, hi2;
    int r0, r1, r2;
    float rH, H3, halfH, Hm1, Hf, Cf, rbound, dt_min, dt_max, far;
};

// Marching state of one ray inside a trip (what the reference keeps in t / last_t / step).
struct RayState {
    float t, last_t;
    uint32_t step;
};

__device__ __forceinline__ float dtf(const MarchParams& a, const RayConsts& c, float t) { return clampf(t * a.dt_gamma, c.dt_min, c.dt_max); }

// Fixed-step lattice arithmetic.  With dt_gamma == 0 (the chair option set) every step adds the same float D, and inside one binade
// [2^e, 2^(e+1)) — where every float is a multiple of u = 2^(e-23) — the rounded sum fl(s + D) is s + Dq with Dq = D rounded to the nearest
// multiple of u, for EVERY s of the binade whose successor stays inside it (the exact sum is s + Dq + r, |r| < u/2, unless D sits exactly
// half-way between two multiples: then round-to-even depends on s and `ok` is false).  So s_k = t + k * Dq, with the product and the sum
// both exact (k * (Dq / u) < 2^24 is part of `ok`), replaces the k-step recurrence, and "first element >= tt" is a rounded quotient
// corrected by two exact comparisons.  Anything else — a window that reaches the binade's top, a tie, dt_gamma != 0 — takes the
// reference's own step-by-step loops.
struct Binade {
    float Dq, rDq, top;
    bool ok;
};
template <int G>
__device__ __forceinline__ Binade binade_of(float t, float D) {
    Binade b;
    const uint32_t bits = __float_as_uint(t);
    const int E = (int)(bits >> 23);         // biased exponent; a negative t has the sign bit here and fails the range test
    const float Ds = scalbnf(D, 150 - E);    // D in units of u: a power-of-two scaling, exact
    const float nf = rintf(Ds);
    b.ok = E > 30 && E < 250 && fabsf(Ds - nf) != 0.5f && nf >= 1.0f && nf * (float)(G + 2) < 16777216.0f;
    b.Dq = scalbnf(nf, E - 150);
    b.rDq = __builtin_amdgcn_rcpf(b.Dq);
    b.top = __uint_as_float((uint32_t)(E + 1) << 23);
    return b;
}
// First k >= k_min with t + k * Dq >= tt, or k_cap + 1 when there is none up to k_cap (all of t + k * Dq, k <= k_cap, lie inside the binade).
__device__ __forceinline__ int lattice_first_at_least(const Binade& b, float t, float tt, int k_min, int k_cap) {
    // NaN tt: fmaxf drops it -> k_min, as the reference's `u < tt` loop (false at once) does
    int k = (int)fminf(fmaxf(ceilf((tt - t) * b.rDq), (float)k_min), (float)(k_cap + 1));
    if (k > k_min && t + (float)(k - 1) * b.Dq >= tt) k--;  // the quotient is off by at most one either way
    else if (k <= k_cap && t + (float)k * b.Dq < tt) k++;
    return k;
}

// `do { t += dt(t); } while (t < tt)` of a one-lane walk: the binade of the current t is kept across calls (a ray crosses a handful of them), the step count is
// the lattice's — at least one step, k = first k >= 1 with t + k * Dq >= tt, the quotient off by one at most and corrected by exact comparisons — and whatever is
// not certainly exact (no fixed step, a tie, a landing at or beyond the binade's top, k beyond the exactness cap k_max) takes the reference's own loop.
// Written with selects: the pre-pass is issue-bound and pays for every exec-mask branch of a hop.
struct LatticeWalk {
    Binade bn{0.f, 0.f, -1.f, false};  // (no binade yet)
    float lo = 0.f, k_max = 0.f;       // t in [lo, bn.top): `bn` is t's binade; k * (Dq / u) < 2^24 up to k_max + 2
};
// largest k for which t + k * Dq is computed exactly from any t of the binade (16777215 = 2^24 - 1 units, two to spare)
__device__ __forceinline__ float lattice_k_cap(const Binade& b, float t) {
    return b.ok ? floorf(16777215.0f / (b.Dq * scalbnf(1.0f, 150 - (int)(__float_as_uint(t) >> 23)))) - 2.0f : 0.0f;
}
__device__ __forceinline__ float advance_past(const MarchParams& a, const RayConsts& c, bool fixed, float D, LatticeWalk& w, float t, float tt) {
    bool stepped = false;
    if (fixed) {
        if (!(t >= w.lo && t < w.bn.top)) {  // entered another binade
            w.bn = binade_of<1>(t, D);
            w.lo = w.bn.top * 0.5f;
            w.k_max = lattice_k_cap(w.bn, t);
        }
        float kf = fminf(fmaxf(ceilf((tt - t) * w.bn.rDq), 1.0f), w.k_max);
        const bool dec = kf > 1.0f && t + (kf - 1.0f) * w.bn.Dq >= tt;
        const bool inc = !dec && t + kf * w.bn.Dq < tt;
        kf = dec ? kf - 1.0f : (inc ? kf + 1.0f : kf);
        const float tn = t + kf * w.bn.Dq;
        stepped = w.bn.ok && kf <= w.k_max && tn < w.bn.top && tn >= tt;  // everything inside the binade: exact
        if (stepped) t = tn;
    }
    if (!stepped)
        do { t += dtf(a, c, t); } while (t < tt);
    return t;
}

// three floats moved by ONE 12-byte access (global_{load,store}_dwordx3 need dword alignment only).  The march kernels are bound by the number
// of accesses the vector L1 processes (TCP_TOTAL_ACCESSES, ~2.2 cycles each per CU however many waves are resident), not by bytes
struct __attribute__((packed, aligned(4))) Float3 {
    float x, y, z;
};
// the part of RayConsts that does not depend on the ray
__device__ __forceinline__ void frame_consts(const MarchParams& a, RayConsts& c) {
    const uint32_t H = a.H, C = a.C;
    c.rH = 1 / (float)H;
    c.H3 = (float)(H * H * H);
    c.halfH = 0.5f * (float)H;
    c.Hm1 = (float)(H - 1);
    c.Hf = (float)H;
    c.Cf = (float)C;
    c.dt_min = 2 * 1.7320508075688772f / a.max_steps;
    c.dt_max = 2 * 1.7320508075688772f * (1 << (C - 1)) / H;
    c.bmin0 = a.bbmin[0]; c.bmin1 = a.bbmin[1]; c.bmin2 = a.bbmin[2];
    c.bmax0 = a.bbmax[0]; c.bmax1 = a.bbmax[1]; c.bmax2 = a.bbmax[2];
    c.hi0 = (float)((double)c.bmax0 - 1e-6); c.hi1 = (float)((double)c.bmax1 - 1e-6); c.hi2 = (float)((double)c.bmax2 - 1e-6);
    c.r0 = a.resolution[0]; c.r1 = a.resolution[1]; c.r2 = a.resolution[2];
    c.rbound = 1 / a.bound;
}
__device__ __forceinline__ void ray_consts(const MarchParams& a, int index, RayConsts& c) {
    const Float3 o = *reinterpret_cast<const Float3*>(a.rays_o + (size_t)index * 3), d = *reinterpret_cast<const Float3*>(a.rays_d + (size_t)index * 3);
    c.ox = o.x; c.oy = o.y; c.oz = o.z;
    c.dx = d.x; c.dy = d.y; c.dz = d.z;
    c.rdx = 1 / c.dx; c.rdy = 1 / c.dy; c.rdz = 1 / c.dz;
    c.far = a.fars[index];
    frame_consts(a, c);
}

// Trip prologue of one ray (raymarching.cu:1163-1172).  Returns false when the ray has nothing to march.
// `resume` (may be null): t left by skip_empty_cells; `last_t` keeps the trip's start.
__device__ __forceinline__ bool ray_start(const MarchParams& a, const RayConsts& c, int index, float noise, const float* resume, RayState& st) {
    float t = a.rays_t[index];
    t += clampf(t * a.dt_gamma, c.dt_min, c.dt_max) * noise;
    st.last_t = t;
    st.step = 0;
    st.t = t;
    if (!(t < c.far)) return false;
    if (resume) st.t = *resume;
    return true;
}

// ---- one point of the sequence.  Sample position at parameter t: clamped onto +-bound in --cut mode (raymarching.cu:1196-1199), onto [bbmin, bbmax - 1e-6] otherwise (:1203-1205).
__device__ __forceinline__ void sample_pos(const MarchParams& a, const RayConsts& c, bool cut, float t, float& x, float& y, float& z) {
    if (cut) {
        x = clampf(c.ox + t * c.dx, -a.bound, a.bound);
        y = clampf(c.oy + t * c.dy, -a.bound, a.bound);
        z = clampf(c.oz + t * c.dz, -a.bound, a.bound);
    } else {
        x = clampf(c.ox + t * c.dx, c.bmin0, c.hi0);
        y = clampf(c.oy + t * c.dy, c.bmin1, c.hi1);
        z = clampf(c.oz + t * c.dz, c.bmin2, c.hi2);
    }
}
// --cut: a point outside the cut box is a static-background sample (found = true, un-warped, :1380-1383); `x < cb[3]` is the reference's own test (:1210)
__device__ __forceinline__ bool inside_cut_box(const float* cb, float x, float y, float z) {
    return x > cb[0] && x < cb[1] && y > cb[2] && x < cb[3] && z > cb[4] && z < cb[5];
}

// Search cell of a sample position: floor((v - bbmin) / hgs) per axis as the reference computes it (IEEE division), without the divisions in the
// common case.  The quotient by reciprocal is within a few 1e-7 relative of the correctly rounded one, so the two can only floor differently when
// the quotient sits within 1e-3 of an integer — then, and for anything not finite, the real division decides.  ONE (rare) branch for the three
// axes: when any of them is in doubt all three are divided, and for an axis that was sure the two floors agree by the same argument.
__device__ __forceinline__ void cell_coords(const MarchParams& a, const RayConsts& c, float x, float y, float z, int& g0, int& g1, int& g2) {
    const float rhgs = __builtin_amdgcn_rcpf(a.hgs);
    const float d0 = x - c.bmin0, d1 = y - c.bmin1, d2 = z - c.bmin2;
    const float q0 = d0 * rhgs, q1 = d1 * rhgs, q2 = d2 * rhgs;
    float f0 = floorf(q0), f1 = floorf(q1), f2 = floorf(q2);
    const float e0 = q0 - f0, e1 = q1 - f1, e2 = q2 - f2;
    const bool sure = e0 >= 1e-3f && e0 <= 0.999f && e1 >= 1e-3f && e1 <= 0.999f && e2 >= 1e-3f && e2 <= 0.999f &&
                      fmaxf(fabsf(q0), fmaxf(fabsf(q1), fabsf(q2))) < 1e6f;
    if (!sure) { f0 = floorf(d0 / a.hgs); f1 = floorf(d1 / a.hgs); f2 = floorf(d2 / a.hgs); }
    g0 = (int)f0; g1 = (int)f1; g2 = (int)f2;
}
__device__ __forceinline__ bool cell_outside(const RayConsts& c, int g0, int g1, int g2) {
    return g0 < 0 || g1 < 0 || g2 < 0 || g0 >= c.r0 || g1 >= c.r1 || g2 >= c.r2;
}
__device__ __forceinline__ int cell_index(const RayConsts& c, int g0, int g1, int g2) { return g2 * c.r1 * c.r0 + g1 * c.r0 + g0; }
__device__ __forceinline__ bool cell_bit(const uint32_t* bits, int i) { return ((bits[i >> 5] >> (i & 31)) & 1u) != 0; }

// Mip level of an un-warped point at parameter t; one cascade: both mip functions clamp to [0, C - 1] = 0.
__device__ __forceinline__ int mip_level(const MarchParams& a, const RayConsts& c, bool one_cascade, float x, float y, float z, float t) {
    return one_cascade ? 0 : max(mip_from_pos(x, y, z, c.Cf), mip_from_dt(dtf(a, c, t), c.Hf, c.Cf));
}
// The density grid's voxel scale on mip level `level`: mip_bound = fminf(2^level, bound) and its reciprocal (1 / 2^level is exact).
__device__ __forceinline__ void mip_scale(const MarchParams& a, const RayConsts& c, int level, float& mip_bound, float& mip_rbound) {
    const float pw = scalbnf(1.0f, level);
    const bool use_pw = pw <= a.bound;
    mip_bound = use_pw ? pw : a.bound;
    mip_rbound = use_pw ? scalbnf(1.0f, -level) : c.rbound;
}

// One voxel hop (raymarching.cu:1386-1428): the density voxel (nx, ny, nz) of the position on its mip level, the parameter distance to the voxel's
// exit face per axis, and their minimum; the chain goes on at the first sequence element >= t + max(0, tmin).  Against the reference's spelling:
//   * (float)(0.5 * (double)v * (double)H) == v * (0.5f * H): both round the exact product once (v has 24 significant bits, H < 2^24);
//   * (n + 0.5f + 0.5f * sign) == n + (0.5f + 0.5f * sign): n is an integer below 2^23 and the addend 0 or 1 — every sum of either form is exact.  The
//     addend is a constant of the ray and the pre-pass's hop a dependent chain, one add per axis shorter this way.
// eval_point (pn_march_window.h) keeps the reference's spelling written out: through this helper, in either spelling, the window and fused kernels
// compiled to other schedules and spill sizes than the parent's and measured 1-2 % slower on the chair (k_march<3, false, 1> 1.6 % with the one-add form).
struct VoxelHop {
    int nx, ny, nz;
    float tx, ty, tz, tmin;
};
__device__ __forceinline__ VoxelHop voxel_hop(const RayConsts& c, float x, float y, float z, float mip_bound, float mip_rbound) {
    VoxelHop v;
    v.nx = (int)clampf((x * mip_rbound + 1) * c.halfH, 0.0f, c.Hm1);
    v.ny = (int)clampf((y * mip_rbound + 1) * c.halfH, 0.0f, c.Hm1);
    v.nz = (int)clampf((z * mip_rbound + 1) * c.halfH, 0.0f, c.Hm1);
    const float sx = 0.5f + 0.5f * signf(c.dx), sy = 0.5f + 0.5f * signf(c.dy), sz = 0.5f + 0.5f * signf(c.dz);
    v.tx = ((((float)v.nx + sx) * c.rH * 2 - 1) * mip_bound - x) * c.rdx;
    v.ty = ((((float)v.ny + sy) * c.rH * 2 - 1) * mip_bound - y) * c.rdy;
    v.tz = ((((float)v.nz + sz) * c.rH * 2 - 1) * mip_bound - z) * c.rdz;
    v.tmin = fminf(v.tx, fminf(v.ty, v.tz));
    return v;
}
__device__ __forceinline__ float hop_target(float t, const VoxelHop& v) { return t + fmaxf(0.0f, v.tmin); }

}  // namespace pnm3
