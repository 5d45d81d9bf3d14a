// Windowed ray march with the inverse-GMLS warp: G lanes per ray (G = 8 or 64), each lane evaluating ONE point of the ray.
//
// The reference loop (raymarching.cu:1121-1434) looks serial — evaluate the sample at t, then either emit it (t += dt) or hop
// to the end of its density voxel (do t += dt while t < tt) — but both branches advance t by the same recurrence
//     s_{k+1} = s_k + clamp(s_k * dt_gamma, dt_min, dt_max)          (float, rounded once per add)
// so the t values a ray can ever visit are the fixed sequence s_0 = t_start, s_1, s_2, ...  Which of them ARE visited depends on
// the evaluations, but the evaluation at s_k (search cell -> nearest IPs -> Newton warps -> blend -> density bit -> voxel exit)
// is a pure function of s_k.  So per round the G lanes of a ray evaluate s_0..s_{G-1} independently, each lane then walks its
// own voxel hop to find the index it would jump to, and every lane replays the visit chain 0 -> jump[0] -> jump[jump[0]] ...
// (G = 8: the 8 jump indices are OR-packed into one dword by DPP; G = 64: the wave-uniform chain is walked with scalar registers and
// v_readlane).  Visited lanes that found an occupied sample write it to the slot given by their rank in the chain.  The round loop is
// wave-uniform: the candidate lists and IP record heads the wave's points need are staged cooperatively in LDS (stage_lists, head_fetch).
//
// Two launches per loop trip use it (pn_march_kernels.h):
//   k_march       G = 8, 8 rays per wave, at most `max_rounds` rounds per ray (2 on a frame's first trip, 1 afterwards): a ray in a
//                 sample-dense region emits its 8 samples in one round.  Rays that are still going after the budget (they graze the
//                 object or have left it and hop through 60-90 voxels without emitting) are appended to a segmented tail list with
//                 their state and ray constants;
//   k_march_tail  G = 64, one wave per listed ray (handed out dynamically, long ones first): 64 sequence elements (~14 voxel hops)
//                 per round, so the critical path of a trip is ~6 rounds instead of ~80 dependent iterations.
// vs. the cooperative form (pn_march_tables.h: 8 lanes share ONE evaluation, one iteration at a time) the results are identical bit
// for bit: same -ffp-contract=off expressions, sequential strict-'<' insertion over the candidate list in the reference's
// visiting order, the `n_IP--` loops replayed literally.
// The t-sequence and the parts of an evaluation that need no candidates are pn_march_seq.h, shared with the skip pre-pass (pn_march_skip.h).
#pragma once
#include "pn_march_seq.h"

#ifndef PN_CAND_FLIGHT
#define PN_CAND_FLIGHT 4  // candidate-list entries a lane has in flight per memory round trip (8: +16 VGPRs, no measurable gain)
#endif
#ifndef PN_HEAD_SPLIT
#define PN_HEAD_SPLIT 0
#endif
#ifndef PN_STAGE_CAP
#define PN_STAGE_CAP 768  // entries per wave: 12 KB (the record heads of a round need 4 * 3 * 64); 4 waves per workgroup, 3 workgroups per CU -> 144 of the 160 KB
#endif

namespace pnm3 {

template <int CTRL>
__device__ __forceinline__ unsigned dpp_u32(unsigned v) {
    return (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, 0xF, 0xF, false);
}

// Timing experiment (-DPN_DBG_PHASES=1 builds only, tools/build_variant.py): per-wave clocks of the phases of a march kernel, summed into
// MarchParams::stats[4 + base ...].  Every phase boundary drains the memory counters, so the phases add up to the wave's lifetime.
#if PN_DBG_PHASES
#define PN_DBG_PHASES_ON 1
struct PhaseClock {
    unsigned long long t0, acc[6];
};
__device__ __forceinline__ unsigned long long dbg_clock() {
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    return __builtin_readcyclecounter();
}
#define PN_PHASE_DECL(pk) pnm3::PhaseClock pk; { for (int _i = 0; _i < 6; _i++) pk.acc[_i] = 0; pk.t0 = pnm3::dbg_clock(); }
#define PN_PHASE(pk, i) do { const unsigned long long _n = pnm3::dbg_clock(); (pk).acc[i] += _n - (pk).t0; (pk).t0 = _n; } while (0)
#define PN_PHASE_FLUSH(pk, stats, base, lane) do { if ((stats) && (lane) == 0) for (int _i = 0; _i < 6; _i++) atomicAdd((stats) + 4 + (base) + _i, (pk).acc[_i]); } while (0)
#define PN_PHASE_ARG , pnm3::PhaseClock& pk
#define PN_PHASE_PASS , pk
#else
#define PN_DBG_PHASES_ON 0
#define PN_PHASE_DECL(pk)
#define PN_PHASE(pk, i)
#define PN_PHASE_FLUSH(pk, stats, base, lane)
#define PN_PHASE_ARG
#define PN_PHASE_PASS
#endif

struct PointEval {
    float x, y, z;  // sample position (warped when IPs were found)
    float dt;       // step at this t
    float tt;       // voxel exit target when the point is not emitted
    bool emit;      // occupied && found
    bool oob;       // search cell outside the spatial hash (error flag of the reference's printf branch)
    unsigned n_cand, n_warp;
};

// First half of one marching iteration at ray parameter t (raymarching.cu:1190-1232): the sample position and the candidate range of
// its search cell.  Split from the rest so that the lanes of a wave can stage the lists they are about to scan together.
struct PointCell {
    float x, y, z;
    bool in_cut, oob;
    int gid, b, e;  // candidates of the search cell: nb[b .. e)  (b == e: none / not searched)
};
__device__ __forceinline__ void point_cell(const MarchParams& a, const March2Tables& tb, const RayConsts& c, float t, PointCell& p) {
    sample_pos(a, c, a.cut, t, p.x, p.y, p.z);
    p.in_cut = true;
    if (a.cut) p.in_cut = inside_cut_box(a.cut_bounds, p.x, p.y, p.z);
    p.oob = false;
    p.gid = -1;
    p.b = p.e = 0;
    if (p.in_cut) {
        // cell_coords (pn_march_seq.h) written out, as is the voxel hop in eval_point: through the shared helpers the same expressions compile to other
        // schedules and spill sizes in the window and fused kernels, and those measured slower
        const float rhgs = __builtin_amdgcn_rcpf(a.hgs);
        const float d0 = p.x - c.bmin0, d1 = p.y - c.bmin1, d2 = p.z - c.bmin2;
        const float q0 = d0 * rhgs, q1 = d1 * rhgs, q2 = d2 * rhgs;
        float f0 = floorf(q0), f1 = floorf(q1), f2 = floorf(q2);
        const float e0 = q0 - f0, e1 = q1 - f1, e2 = q2 - f2;
        const bool sure = e0 >= 1e-3f && e0 <= 0.999f && e1 >= 1e-3f && e1 <= 0.999f && e2 >= 1e-3f && e2 <= 0.999f &&
                          fmaxf(fabsf(q0), fmaxf(fabsf(q1), fabsf(q2))) < 1e6f;
        if (!sure) { f0 = floorf(d0 / a.hgs); f1 = floorf(d1 / a.hgs); f2 = floorf(d2 / a.hgs); }
        const int g0 = (int)f0, g1 = (int)f1, g2 = (int)f2;
        p.oob = (g0 < 0 || g1 < 0 || g2 < 0 || g0 >= c.r0 || g1 >= c.r1 || g2 >= c.r2);
        if (!p.oob) {
            p.gid = cell_index(c, g0, g1, g2);
            const int2 rng = tb.nb_rng[p.gid];
            p.b = rng.x;
            p.e = rng.y;
        }
    }
}

// Wave-cooperative staging of candidate lists in LDS.  The lanes of a wave scan a handful of DISTINCT lists per round (the 8 lanes of a
// ray sit in the same search cell or two; in the tail pass 64 points of one ray cross four or five cells), but every lane used to fetch
// its list itself: ~30 of the ~58 vector-memory instructions of a wave-round, each a 64-lane x 16 B gather.  Measured (rocprofv3
// VmemLatency): 2 400 cycles per vector-memory instruction with the chip full of march waves against 560 when nearly empty — the vector
// L1 path was the bottleneck, not HBM and not the ALUs.  Here each distinct list is copied once, by all 64 lanes with coalesced 16-byte
// LDS-DMA loads (global_load_lds_dwordx4: no staging registers, one wait for all lists), and the per-lane scans read LDS.
// Must be called with all 64 lanes active (destination = wave-uniform base + lane * 16).  Returns this lane's list offset in `stage`
// (entries), or -1 when the wave's lists did not all fit: those lanes scan from global memory as before.
__device__ __forceinline__ void glds16(const float4* g, float4* l) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g, (__attribute__((address_space(3))) void*)l, 16, 0, 0);
}
template <int CAP = PN_STAGE_CAP>
__device__ __forceinline__ int stage_lists(float4* stage, const float4* __restrict__ nb, int b, int len, int lane) {
    int my_off = -1;
    int cursor = 0;
    unsigned long long todo = __ballot(len > 0);
    while (todo) {  // one iteration per distinct list (lists are per cell: same start <=> same list)
        const int leader = __builtin_ctzll(todo);
        const int lb = __builtin_amdgcn_readlane(b, leader), ll = __builtin_amdgcn_readlane(len, leader);
        const bool mine = len > 0 && b == lb;
        todo &= ~__ballot(mine);
        if (cursor + ll > CAP) continue;
        if (mine) my_off = cursor;
        for (int i0 = 0; i0 < ll; i0 += 64)
            if (i0 + lane < ll) glds16(nb + lb + i0 + lane, stage + cursor + i0);
        cursor += ll;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    return my_off;
}

// Candidate search of one marching iteration, one lane (raymarching.cu:1232-1244 -> find_closest_IP(s)): the K nearest IPs of the point,
// nearest first, -1 = none.  `stage` / `my_off`: this lane's candidate list in LDS (stage_lists), my_off < 0: read it from tb.nb.
template <int K>
__device__ __forceinline__ void eval_scan(const MarchParams& a, const March2Tables& tb, const PointCell& pc, const float4* stage, int my_off, int (&ips)[3],
                                          unsigned& n_cand) {
    const float x = pc.x, y = pc.y, z = pc.z;
    ips[0] = ips[1] = ips[2] = -1;
    n_cand = 0;
    if (pc.in_cut && !pc.oob) {
        {
            const int n_list = pc.e - pc.b;
            n_cand = (unsigned)n_list;
            if (K == 1) {
                // find_closest_IP (:986-1043): own cell first, the 26 neighbours only if that found nothing; `d < best` from 9999.9
                const int own = a.pig_cnt[pc.gid];
                float best = (float)9999.9;
                auto scan1 = [&](const float4* base) {
                    for (int j = 0; j < own; j++) {
                        const float4 v = base[j];
                        const float ax = v.x - x, ay = v.y - y, az = v.z - z;
                        const float d = ax * ax + ay * ay + az * az;
                        if (d < best) { best = d; ips[0] = __float_as_int(v.w); }
                    }
                    if (ips[0] == -1) {
                        for (int j = own; j < n_list; j++) {
                            const float4 v = base[j];
                            const float ax = v.x - x, ay = v.y - y, az = v.z - z;
                            const float d = ax * ax + ay * ay + az * az;
                            if (d < best) { best = d; ips[0] = __float_as_int(v.w); }
                        }
                    }
                };
                if (my_off >= 0) scan1(stage + my_off); else scan1(tb.nb + pc.b);
            } else {
                // find_closest_IPs (:1045-1118): all 27 cells in visiting order (= list order), insertion on strict '<'.  Written as selects
                // on the three comparisons (d0 <= d1 <= d2 always, so d < d0 implies d < d1 implies d < d2 and the reference's
                // if / else-if chain is exactly this): the compiler's branchy form of the chain cost ~55 instructions and four
                // exec-mask branches per candidate, this one 21 and none.  The IP id travels with the distance, so the selected
                // entries need no second fetch.
                // Round 3: the three running minima are 64-bit KEYS (distance bits << 32 | position in the list), compared as doubles: for
                // non-negative floats the bit pattern orders like the value, the position breaks ties towards the earlier candidate — exactly the
                // sequential strict-'<' insertion — and any such pattern is a finite positive double (a float's exponent field never fills the
                // double's), so v_min_f64 / v_max_f64 order the keys: five instructions per candidate instead of thirteen selects (a wave pays for
                // its longest list, ~60 entries in the dense cells: the scan is more than half of pass 1's VALU instructions).  The ids of the
                // winners are read back from the list afterwards.  Sentinel = (FLT_MAX bits, 0): a candidate at distance FLT_MAX, inf or NaN
                // never enters, as `d < FLT_MAX` never holds for it.
                const double sent = __hiloint2double(0x7F7FFFFF, 0);
                double m0 = sent, m1 = sent, m2 = sent;
                auto kmin = [](double a_, double b_) { double r; asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a_), "v"(b_)); return r; };
                auto kmax = [](double a_, double b_) { double r; asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a_), "v"(b_)); return r; };
                auto insert = [&](const float4& v, int pos, bool valid) {
                    const float ax = v.x - x, ay = v.y - y, az = v.z - z;
                    const float d = ax * ax + ay * ay + az * az;
                    const double k = valid ? __hiloint2double(__float_as_int(d), pos) : sent;
                    const double t0 = kmax(m0, k);
                    m0 = kmin(m0, k);
                    if (K > 2) {
                        const double t1 = kmax(m1, t0);
                        m1 = kmin(m1, t0);
                        m2 = kmin(m2, t1);
                    } else {
                        m1 = kmin(m1, t0);
                    }
                };
                auto scan = [&](const float4* base) {  // entries base[0 .. n_list)
                    int j0 = 0;
                    for (; j0 + PN_CAND_FLIGHT <= n_list; j0 += PN_CAND_FLIGHT) {  // entries in flight per round trip
                        float4 v[PN_CAND_FLIGHT];
#pragma unroll
                        for (int u = 0; u < PN_CAND_FLIGHT; u++) v[u] = base[j0 + u];
#pragma unroll
                        for (int u = 0; u < PN_CAND_FLIGHT; u++) insert(v[u], j0 + u, true);
                    }
                    if (j0 < n_list) {
                        float4 v[PN_CAND_FLIGHT - 1];
#pragma unroll
                        for (int u = 0; u < PN_CAND_FLIGHT - 1; u++) v[u] = base[min(j0 + u, n_list - 1)];
#pragma unroll
                        for (int u = 0; u < PN_CAND_FLIGHT - 1; u++) insert(v[u], j0 + u, j0 + u < n_list);
                    }
                    // a key still at the sentinel's distance bits found nothing (FLT_MAX itself is never inserted)
                    const int h0 = __double2hiint(m0), h1 = __double2hiint(m1), h2 = __double2hiint(m2);
                    if (h0 != 0x7F7FFFFF) ips[0] = __float_as_int(base[__double2loint(m0)].w);
                    if (h1 != 0x7F7FFFFF) ips[1] = __float_as_int(base[__double2loint(m1)].w);
                    if (K > 2 && h2 != 0x7F7FFFFF) ips[2] = __float_as_int(base[__double2loint(m2)].w);
                };
                if (my_off >= 0) scan(stage + my_off); else scan(tb.nb + pc.b);
            }
        }
    }
}

// The selected IPs' record heads (p_ori, p_def, F^-1: 64 B each) for all 64 lanes at once.  Per lane they are three scattered 64-byte
// records; fetched lane by lane (3 x 4 global_load_dwordx4) every instruction costs the vector L1 one access per LANE (~770 per wave-round,
// a third of all the kernel's accesses, and the accesses are what bounds it).  Here the four lanes of a quad fetch each other's records:
// instruction (k, j) has every lane load part (lane & 3) of the k-th record of lane j of its quad — one contiguous 64 B per quad, 16
// accesses per instruction — by LDS-DMA into stage[(k * 4 + j) * 64 + lane]; lane (Q, j) then reads its four parts back from
// stage[(k * 4 + j) * 64 + Q * 4 ...].  All 64 lanes must be active; lanes without an IP fetch record 0.  Needs 4 * K * 64 entries of `stage`
// (the candidate lists staged there have been consumed by then).
template <int CTRL>
__device__ __forceinline__ int dpp_i32(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true); }
template <int K, int SPLIT = PN_HEAD_SPLIT>
__device__ __forceinline__ void head_fetch(float4* stage, const float4* __restrict__ rec, const int (&ips)[3], int lane, float4 (&rh)[3][4]) {
    const int q = lane & 3;
    // SPLIT = 1: the first two records, then the third, through the same 8 KB (one more round trip per round, a third less LDS per wave)
    constexpr int K0 = (SPLIT && K > 2) ? 2 : K;
#pragma unroll
    for (int pass = 0; pass < ((K0 < K) ? 2 : 1); pass++) {
        const int kb = pass ? K0 : 0, ke = pass ? K : K0;
#pragma unroll
        for (int k = kb; k < ke; k++) {
            const int ipk = ips[k] >= 0 ? ips[k] : (ips[0] >= 0 ? ips[0] : 0);
            const int i0 = dpp_i32<0x00>(ipk), i1 = dpp_i32<0x55>(ipk), i2 = dpp_i32<0xAA>(ipk), i3 = dpp_i32<0xFF>(ipk);  // quad_perm broadcasts
            glds16(rec + (size_t)i0 * PN_REC_VEC4 + q, stage + ((k - kb) * 4 + 0) * 64);
            glds16(rec + (size_t)i1 * PN_REC_VEC4 + q, stage + ((k - kb) * 4 + 1) * 64);
            glds16(rec + (size_t)i2 * PN_REC_VEC4 + q, stage + ((k - kb) * 4 + 2) * 64);
            glds16(rec + (size_t)i3 * PN_REC_VEC4 + q, stage + ((k - kb) * 4 + 3) * 64);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
        for (int k = kb; k < ke; k++) {
            const float4* h = stage + ((k - kb) * 4 + q) * 64 + (lane & ~3);
#pragma unroll
            for (int u = 0; u < 4; u++) rh[k][u] = h[u];
        }
        if (K0 < K) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the reads above complete before the region is overwritten
    }
}

// Rest of one marching iteration, one lane: pre-filter, inverse warps, blend, density bit, voxel exit (raymarching.cu:1246-1431).
template <int K, bool MULTI>
__device__ __forceinline__ void eval_point(const MarchParams& a, const March2Tables& tb, const RayConsts& c, float t, const PointCell& pc,
                                           const int (&ips)[3], const float4 (&rh)[3][4], unsigned n_cand, PointEval& r) {
    bool found = false;
    float x = pc.x, y = pc.y, z = pc.z;
    r.oob = pc.oob;
    r.n_cand = n_cand;
    r.n_warp = 0;
    if (pc.in_cut) {
        float x_map = 0.0f, y_map = 0.0f, z_map = 0.0f;
        int n_IP = (ips[0] != -1) + (ips[1] != -1) + (ips[2] != -1);
        found = n_IP > 0;
        if (found) {
            // the selected IPs' record heads (p_ori, p_def, F^-1: 64 B each) arrive in rh[][] (head_fetch below) — the pre-filter loop, whose
            // bound shrinks as it runs, and the first Newton step work on registers
            // pre-filter (:1246-1251) on the candidates' deformed positions: `n_IP--` inside the loop it bounds, strict '<' on z only
#pragma unroll
            for (int k = 0; k < K; k++) {
                if (k < n_IP) {
                    const float cx = rh[k][0].w, cy = rh[k][1].x, cz = rh[k][1].y;  // p_def
                    if (cx <= c.bmin0 || cy <= c.bmin1 || cz < c.bmin2 || cx >= c.bmax0 || cy >= c.bmax1 || cz >= c.bmax2) n_IP--;
                }
            }
            if (n_IP <= 0) found = false;
            if (found) {
                float ps[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, dk[3] = {0, 0, 0};
                // per-IP Newton warp (:1262-1324): a rejected result still fills its slot and shrinks the bound
#pragma unroll
                for (int k = 0; k < K; k++) {
                    if (k < n_IP) {
                        float pw[3];
                        r.n_warp++;
                        const float4* __restrict__ rp = tb.rec + (size_t)ips[k] * PN_REC_VEC4;
                        if (warp_record<MULTI>(rh[k], rp, a.max_iter_num, a.IP_dx, x, y, z, pw, &dk[k])) n_IP--;
                        ps[3 * k] = pw[0]; ps[3 * k + 1] = pw[1]; ps[3 * k + 2] = pw[2];
                    }
                }
                if (n_IP == 1) {
                    x_map = ps[0]; y_map = ps[1]; z_map = ps[2];
                } else if (n_IP == 2) {
                    const float dist_sum = dk[0] + dk[1];
                    const float w0 = dk[1] / dist_sum, w1 = dk[0] / dist_sum;
                    x_map = w0 * ps[0] + w1 * ps[3];
                    y_map = w0 * ps[1] + w1 * ps[4];
                    z_map = w0 * ps[2] + w1 * ps[5];
                } else if (n_IP == 3) {
                    const float dist_sum = dk[0] * dk[1] + dk[1] * dk[2] + dk[2] * dk[0];
                    const float w0 = dk[1] * dk[2] / dist_sum;
                    const float w1 = dk[0] * dk[2] / dist_sum;
                    const float w2 = dk[0] * dk[1] / dist_sum;
                    x_map = w0 * ps[0] + w1 * ps[3] + w2 * ps[6];
                    y_map = w0 * ps[1] + w1 * ps[4] + w2 * ps[7];
                    z_map = w0 * ps[2] + w1 * ps[5] + w2 * ps[8];
                }
                x = x_map; y = y_map; z = z_map;  // n_IP == 0 here maps the sample to the origin (:1372-1374)
            }
        }
    } else {
        found = true;  // cut mode, outside the cut box: un-warped background sample (:1380-1383)
    }

    const float dt = dtf(a, c, t);
    // one cascade: both mip functions clamp to [0, C - 1] = 0
    const int level = (c.Cf == 1.0f) ? 0 : max(mip_from_pos(x, y, z, c.Cf), mip_from_dt(dt, c.Hf, c.Cf));
    // mip_scale and voxel_hop (pn_march_seq.h) written out in the reference's order and spelling, see point_cell
    const float pw2 = scalbnf(1.0f, level);
    const bool use_pw = pw2 <= a.bound;
    const float mip_bound = use_pw ? pw2 : a.bound;
    const float mip_rbound = use_pw ? scalbnf(1.0f, -level) : c.rbound;
    const int nx = (int)clampf((x * mip_rbound + 1) * c.halfH, 0.0f, c.Hm1);
    const int ny = (int)clampf((y * mip_rbound + 1) * c.halfH, 0.0f, c.Hm1);
    const int nz = (int)clampf((z * mip_rbound + 1) * c.halfH, 0.0f, c.Hm1);
    bool occ = false;
    if (found) {  // the occupancy bit only matters when an IP was found (`occ && found`)
        const uint32_t vox = (uint32_t)(level * c.H3 + (float)morton3D(nx, ny, nz));
        occ = (bool)(a.grid[vox / 8] & (1 << (vox % 8)));
    }
    r.emit = occ && found;
    r.x = x; r.y = y; r.z = z;
    r.dt = dt;
    const float tx = (((nx + 0.5f + 0.5f * signf(c.dx)) * c.rH * 2 - 1) * mip_bound - x) * c.rdx;
    const float ty = (((ny + 0.5f + 0.5f * signf(c.dy)) * c.rH * 2 - 1) * mip_bound - y) * c.rdy;
    const float tz = (((nz + 0.5f + 0.5f * signf(c.dz)) * c.rH * 2 - 1) * mip_bound - z) * c.rdz;
    r.tt = t + fmaxf(0.0f, fminf(tx, fminf(ty, tz)));
}

// Up to `max_rounds` windows of G sequence elements of one ray; the G lanes [gbase, gbase + G) run in lock step.
// Returns true when the ray is done for this trip (t >= far, or n_step samples), false when the round budget ran out; `st` is
// advanced either way (identically on all G lanes).  Samples go to xyzs/dirs/deltas[slot], slot = number emitted before.
// Called by ALL 64 lanes of the wave (have_ray = false for the lanes of a group without a ray): the round loop is wave-uniform so that
// the candidate lists of a round can be staged cooperatively (stage_lists) in `stage`, the wave's CAP entries of LDS (CAP >= 512; below 768 the three
// record heads of a lane go through it in two passes: SPLIT).
template <int K, bool MULTI, int G, int CAP = PN_STAGE_CAP, int SPLIT = PN_HEAD_SPLIT>
__device__ inline bool march_window(const MarchParams& a, const March2Tables& tb, const RayConsts& c, uint32_t n_step, int sub, int gbase, int lane,
                                    float4* stage, float* __restrict__ xyzs, float* __restrict__ dirs, float* __restrict__ deltas, RayState& st,
                                    int max_rounds, bool have_ray PN_PHASE_ARG) {
    float t = st.t, last_t = st.last_t;
    uint32_t step = st.step;
    const float far = c.far;
    unsigned st_iter = 0, st_cand = 0, st_warp = 0;  // instrumentation (visited points only), reported when a.stats != nullptr
    bool done = true;
    bool running = have_ray;
    int rounds = 0;
    const bool fixed = a.dt_gamma == 0.0f;
    const float D = clampf(0.0f, c.dt_min, c.dt_max);  // dtf() of any finite t when dt_gamma == 0
    while (true) {
        bool go = running && t < far && step < n_step;  // the same on the G lanes of a ray
        if (go && rounds == max_rounds) { done = false; go = false; }
        running = go;
        if (!__any(go)) break;
        rounds++;
        // this lane's point s_sub and its successor
        Binade bn;
        bn.Dq = bn.rDq = bn.top = 0.f; bn.ok = false;
        bool fast = false;  // the whole window s_0 .. s_G lies inside t's binade: lattice arithmetic
        float s = 0.f, nxt = 0.f;
        bool active = false;
        PointCell pc;
        pc.x = pc.y = pc.z = 0.f; pc.in_cut = false; pc.oob = false; pc.gid = -1; pc.b = pc.e = 0;
        if (go) {
            if (fixed) {
                // (G == 1, one lane per ray: the lattice reaches 64 elements ahead, so that a voxel hop is one product instead of a stepping loop)
                bn = binade_of<(G == 1 ? 64 : G)>(t, D);
                fast = bn.ok && t + (float)(G == 1 ? 65 : G) * bn.Dq < bn.top;
            }
            if (fast) {
                s = t + (float)sub * bn.Dq;
                nxt = t + (float)(sub + 1) * bn.Dq;
            } else {
                s = t;
                for (int j = 0; j < G - 1; j++)
                    if (j < sub) s += dtf(a, c, s);
                nxt = s + dtf(a, c, s);
            }
            active = s < far;
            if (active) point_cell(a, tb, c, s, pc);
        }
        PN_PHASE(pk, 1);
        // a window none of whose points has a candidate (rays that have left the object and walk on to `far`, grazing rays between two parts of
        // it) needs no lists, no scan and no record heads: what is left of the round is the voxel arithmetic and the chain
        const bool any_list = __any(pc.e != pc.b);
        int my_off = -1;
        if (any_list) my_off = stage_lists<CAP>(stage, tb.nb, pc.b, pc.e - pc.b, lane);
        PN_PHASE(pk, 2);
        PointEval ev;
        ev.emit = false; ev.oob = false; ev.tt = 0.f; ev.dt = 0.f; ev.x = ev.y = ev.z = 0.f; ev.n_cand = 0; ev.n_warp = 0;
        int ips[3] = {-1, -1, -1};
        unsigned n_cand = 0;
        float4 rh[3][4];
#pragma unroll
        for (int k = 0; k < 3; k++)
#pragma unroll
            for (int u = 0; u < 4; u++) rh[k][u] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (any_list) {
            if (go && active) eval_scan<K>(a, tb, pc, stage, my_off, ips, n_cand);
            head_fetch<K, SPLIT>(stage, tb.rec, ips, lane, rh);
        }
        if (go && active) eval_point<K, MULTI>(a, tb, c, s, pc, ips, rh, n_cand, ev);
        PN_PHASE(pk, 3);
        if (go) {
            // where the chain goes from this point: the next element (emitted) or the first element not below the voxel exit;
            // G = first element of the next window, G + 1 = beyond it
            int jump = sub + 1;
            float t_hop = nxt;  // G == 1: where the chain goes from this (visited) point
            if (G == 1 && active && !ev.emit) {
                if (fast) {
                    const int k = lattice_first_at_least(bn, t, ev.tt, 1, 64);
                    t_hop = t + (float)min(k, 64) * bn.Dq;       // exact: inside the binade
                    if (k > 64) while (t_hop < ev.tt) t_hop += dtf(a, c, t_hop);
                } else {
                    while (t_hop < ev.tt) t_hop += dtf(a, c, t_hop);  // do { t += dt } while (t < tt): the first step is `nxt`
                }
            } else if (active && !ev.emit) {
                if (fast) {
                    jump = lattice_first_at_least(bn, t, ev.tt, sub + 1, G);
                } else {
                    float u = nxt;
                    int k = sub + 1;
                    while (k < G && u < ev.tt) { u += dtf(a, c, u); k++; }
                    jump = (k == G && u < ev.tt) ? G + 1 : k;
                }
            }
            unsigned word = 0;
            if (G == 8) {
                word = (unsigned)jump << (4 * sub);
                word |= dpp_u32<0xB1>(word);   // lane ^ 1
                word |= dpp_u32<0x4E>(word);   // lane ^ 2
                word |= dpp_u32<0x141>(word);  // lane <-> 7 - lane within each 8
            }
            const unsigned long long gmask = (G == 64) ? ~0ull : ((1ull << G) - 1ull);
            const unsigned long long emitm = (__ballot(ev.emit) >> gbase) & gmask;
            const unsigned long long actm = (__ballot(active) >> gbase) & gmask;
            // replay of the visit chain, identically on the G lanes
            int cur = 0, prev_emit = -1, n_emit = 0, last_vis = 0;
            int my_ord = -1, my_prev = -1;
            bool visited = false, ended = false;
            if (G == 1) {
                // one ray per lane: its single point is the visited one
                if (!active) ended = true;
                else {
                    visited = true; my_ord = 0; my_prev = -1; last_vis = 0;
                    if (ev.emit) { prev_emit = 0; n_emit = 1; if (step + 1u == n_step) ended = true; }
                }
            } else if (G == 64) {
                // one ray per wave: the chain is wave-uniform — walked with scalar registers and v_readlane instead of 64 lanes each
                // following it through ds_bpermute (~14 dependent LDS round trips per round)
                unsigned long long vis = 0ull;
                const int need = (int)(n_step - step);
                while (cur < 64) {
                    if (!((actm >> cur) & 1ull)) { ended = true; break; }
                    vis |= 1ull << cur;
                    last_vis = cur;
                    if ((emitm >> cur) & 1ull) {
                        prev_emit = cur;
                        n_emit++;
                        if (n_emit == need) { ended = true; break; }
                    }
                    cur = __builtin_amdgcn_readlane(jump, cur);
                }
                const unsigned long long ev_m = vis & emitm, below = (1ull << sub) - 1ull;
                visited = ((vis >> sub) & 1ull) != 0;
                my_ord = (int)__popcll(ev_m & below);
                my_prev = (ev_m & below) ? 63 - (int)__clzll(ev_m & below) : -1;
            } else {
            while (cur < G) {
                if (!((actm >> cur) & 1ull)) { ended = true; break; }  // s_cur >= far: the march is over
                if (cur == sub) { visited = true; my_ord = n_emit; my_prev = prev_emit; }
                last_vis = cur;
                const bool em = (emitm >> cur) & 1ull;
                const int nx_idx = (int)((word >> (4 * cur)) & 0xFu);
                if (em) {
                    prev_emit = cur;
                    n_emit++;
                    if (step + (uint32_t)n_emit == n_step) { ended = true; break; }
                }
                cur = nx_idx;
            }
            }
            // emitted samples: slot = step + rank in the chain; deltas[1] = t_after - last_t (raymarching.cu:1395-1410)
            const float prev_nxt = __shfl(nxt, gbase + max(my_prev, 0));
            if (visited) {
                st_iter++; st_cand += ev.n_cand; st_warp += ev.n_warp;
                if (ev.oob && a.err_flag) atomicOr(a.err_flag, 1);
                if (ev.emit) {
                    const uint32_t slot = step + (uint32_t)my_ord;
                    float* X = xyzs + (size_t)slot * 3;
                    float* Dd = dirs + (size_t)slot * 3;
                    float* L = deltas + (size_t)slot * 2;
                    *reinterpret_cast<Float3*>(X) = Float3{ev.x, ev.y, ev.z};
                    if (dirs) *reinterpret_cast<Float3*>(Dd) = Float3{c.dx, c.dy, c.dz};   // (nullptr: a caller that keeps the rays' directions itself)
                    *reinterpret_cast<float2*>(L) = make_float2(ev.dt, nxt - (my_prev >= 0 ? prev_nxt : last_t));
                }
            }
            // (G == 64: wave-uniform lane indices — v_readlane instead of a ds_bpermute round trip)
            const float last_emit_nxt = (G == 64) ? __int_as_float(__builtin_amdgcn_readlane(__float_as_int(nxt), max(prev_emit, 0))) : __shfl(nxt, gbase + max(prev_emit, 0));
            if (n_emit > 0) last_t = last_emit_nxt;
            step += (uint32_t)n_emit;
            // next window start: s_G, or further when the last visited point's voxel exit lies beyond the window
            const float sG = (G == 64) ? __int_as_float(__builtin_amdgcn_readlane(__float_as_int(nxt), 63)) : __shfl(nxt, gbase + G - 1);
            const float tt_last = (G == 64) ? __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ev.tt), last_vis)) : __shfl(ev.tt, gbase + last_vis);
            if (ended) {
                running = false;  // done for this trip; t is not needed any more (composite tracks rays_t itself)
            } else if (G == 1) {
                t = t_hop;
            } else {
                t = sG;
                if (cur == G + 1)
                    while (t < tt_last) t += dtf(a, c, t);
            }
        }
        PN_PHASE(pk, 4);
    }
#if !PN_DBG_PHASES  // (the phase-clock build reuses the counter block and must not be disturbed by these atomics)
    if (a.stats) {
        if (st_iter) { atomicAdd(a.stats, (unsigned long long)st_iter); atomicAdd(a.stats + 1, (unsigned long long)st_cand); }
        if (st_warp) atomicAdd(a.stats + 2, (unsigned long long)st_warp);
    }
#endif
    st.t = t;
    st.last_t = last_t;
    st.step = step;
    return done;
}

}  // namespace pnm3
