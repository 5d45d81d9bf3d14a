// The skip pre-pass in front of the windowed march (k_march_skip, pn_march_kernels.h), ONE lane per ray: the leading run of marching iterations that can
// neither emit nor warp — search cells whose 27-neighbourhood holds no IP and, in --cut mode, static-background points (outside the cut box) in empty
// density voxels.  In --cut mode every ray crosses the whole +-bound volume, so without this pre-pass all of those iterations went through the 8-lane /
// wave-per-ray kernels (trex option set at 1008x756: 65.7 M visited points per frame).  At 800x800 ~86 % of the first trip's iterations are of this kind
// (rays crossing the empty part of the IP bounding box): no candidate is found, the sample is not warped, the only memory touched is the cell's list range.
// skip_empty_cells returns the t at which the windowed march has to take over (first iteration whose cell has candidates, or t >= far); the arithmetic is
// the windowed march's own (pn_march_seq.h), so resuming there is bit-identical to having run every iteration in the windowed march.
//
// THE HOP.  The kernel's duration is its longest lane's chain (~130 hops of ~230 dependent instructions, 0.7 us each for a lone wave), so the hop is kept short:
// the cell coordinates without divisions, one cascade without the mip functions, with a fixed step the do-while that advances t past the voxel exit replaced
// by lattice arithmetic (advance_past), and the emptiness test one LDS bit per search cell instead of a dependent global round trip every third hop or so.
//
// THE LOOK-AHEADS.  The rays that graze the object do up to ~85 hops across cells in which nothing can happen (65 of the pre-pass's 77 us were its longest such
// walk), and with --cut every ray hops through the static background's empty space (~86 hops per ray on the trex option set, and the pre-pass is issue-bound on
// them: 12 k waves; keeping the bitfield's block map in LDS so that a hop waits for no load moved nothing).  All the caller needs is an element of the ray's
// t-sequence that the reference's chain certainly visits just before something can happen, and two facts make it computable without walking:
//   * the t-sequence is grid-independent whatever the chain visits of it — a lattice with a fixed step (Binade), five instructions per element otherwise, where
//     visiting one costs 230 — and WHICH elements the chain visits is local (certainly_visited, below);
//   * a DDA knows which cells the ray crosses.  It goes on while the next cell is one in which nothing can happen, minding the crossings that lie within 2e-3
//     cell widths of another face, where the reference's float arithmetic could mean a lateral neighbour.
// The chain is restarted at the last certainly-visited element more than a margin before the stopping face (none: the hops go on from where they were) and the
// exact hops take over; if the DDA reaches `far` the chain emits nothing.
//   Without --cut (cell_dda; fixed step, one cascade, bound <= 1): the cells are the search grid's, "nothing can happen" = no candidates (cell_bits), a start
//   next to a face asks the one-cell neighbourhood map (cell_bits2).  ONE attempt per ray, before the loop, so that the lanes of a wave stay together.
//   With --cut (region_dda): a REGION is one 8^3-voxel block of the top cascade level (a 64-byte line of the bitfield; the caller may choose 4^3); its bit says
//   "interesting": some voxel of it is occupied on ANY level >= L that a point inside it can be tested on (one map per L: a ray asks the map of the lowest level
//   its dt still allows), or it meets the cut box (inside which the search cells decide).  A point in a region without the bit is a static-background sample in
//   an empty voxel whatever its mip level: the chain emits nothing there.  The restart pair (p, e) must also have every element of the t-sequence within one
//   top-level voxel diagonal before p on p's mip level: an element v <= p whose voxel (on v's level) contains p is then on p's level, so it is p's voxel, its
//   exit is exit(p) to rounding, and the chain lands on the first element behind it: e.  Behind an interesting region without an event the look-ahead is
//   repeated after PN_REGION_RETRY_HOPS exact hops.
//
// THE HOP BUDGET (> 0, with the cell look-ahead): a wave is as slow as its slowest ray, and 0.04 % of the rays (face-hugging or axis-parallel ones: ~270 of
// 640 000, spread over a fifth of the busy waves) still walk 40-80 hops; after `hop_budget` hops the pre-pass hands the ray — standing on a visited element
// like any other resume point — to the windowed march, which evaluates 64 elements (~14 hops) per round and has 12 000 other rays to hide it behind.
#pragma once
#include "pn_march_seq.h"

#ifndef PN_REGION_RETRY_HOPS
#define PN_REGION_RETRY_HOPS 6   // exact hops behind a region look-ahead before the next one (measured alone on trex: 2 / 6 / 10 / 16 / 24 hops -> 201 / 175 / 178 / 185 / 205 us; hop by hop 285)
#endif

namespace pnm3 {

// ---- restarting the chain at an element it certainly visits.
// WHICH elements the chain visits is local: from any visited element of a voxel V it computes tt ~ the parameter at which the ray leaves V and lands on the first
// element >= tt.  So an element e is visited whenever its predecessor p lies safely inside its voxel (p < tt_p - margin, tt_p = the chain's own exit expression
// evaluated at p: voxel_hop) and e lies safely behind that exit (e >= tt_p + margin): whichever element of p's voxel the chain is on, it computes an exit within
// the margin of tt_p and lands on e (and if an ambiguity further back made it skip p's voxel, it landed on the first element behind p: e again).
// The margins, in units of t: ~60 ulp of t plus the error of (face - x) * (1 / d) for the axis in question (an axis the ray is nearly parallel to has a huge
// 1 / d, but its face is never the nearest one; where it is, beyond RD_MAX, there is no restart).
constexpr float VOX_MARGIN_T = 3e-5f, VOX_MARGIN_RD = 2e-6f;    // around a voxel's exit: per max(1, |t|), per 1 / |d| of the exit axis
constexpr float FACE_MARGIN_T = 2e-4f, FACE_MARGIN_RD = 1e-5f;  // in front of the face a DDA stopped at: elements this far before it are in the cells it crossed
constexpr float RD_MAX = 1e3f;
// a crossing point this close to another face, in cell (region) widths: the reference's float cell arithmetic, errors ~1e-6 widths, may mean the lateral neighbour
constexpr float FACE_DOUBT_LO = 2e-3f, FACE_DOUBT_HI = 0.998f;
__device__ __forceinline__ bool face_clear(float u) { return u >= FACE_DOUBT_LO && u <= FACE_DOUBT_HI; }

// m_face for a DDA's stopping face on axis m; `t_scale`: the parameter whose magnitude sizes the ulp term.  `rd` = 1 / |d| of that axis.
__device__ __forceinline__ float face_margin(const RayConsts& c, int m, float t_scale, float& rd) {
    const float rdx = c.rdx, rdy = c.rdy, rdz = c.rdz;  // (copies: a conditional over the members themselves selects an address and keeps `c` in memory)
    rd = fabsf(m == 0 ? rdx : (m == 1 ? rdy : rdz));
    return FACE_MARGIN_T * fmaxf(1.0f, fabsf(t_scale)) + FACE_MARGIN_RD * fminf(rd, RD_MAX);
}
// Is e, whose predecessor p has the sample position (x, y, z) on the mip level of (mip_bound, mip_rbound), certainly visited?
__device__ __forceinline__ bool certainly_visited(const RayConsts& c, float p, float e, float t_scale, float x, float y, float z, float mip_bound,
                                                  float mip_rbound) {
    const VoxelHop v = voxel_hop(c, x, y, z, mip_bound, mip_rbound);
    const float rdx = c.rdx, rdy = c.rdy, rdz = c.rdz;
    const float rd_min = fabsf(v.tmin == v.tx ? rdx : (v.tmin == v.ty ? rdy : rdz));
    const float m_vox = VOX_MARGIN_T * fmaxf(1.0f, fabsf(t_scale)) + VOX_MARGIN_RD * rd_min;
    const float ttp = hop_target(p, v);
    return rd_min < RD_MAX && p < ttp - m_vox && e >= ttp + m_vox && e < c.far;
}

// Where a ray can stop.  A sample is only ever emitted at a point whose search cell has candidates, so beyond the last such cell on its way
// a ray does nothing but hop from voxel to voxel until `far` — for a ray that misses the object but crosses its bounding box that is ALL it
// does (most of k_march_skip's work), and a ray that has left the object behind walks on through the tail pass (the longest tail rays).
// `bits2` marks the cells within one cell of a cell with candidates (k_frame_prologue); the ray is sampled backwards from `far` every 0.9 cell
// lengths, and the march may end at the last sample before the first marked one: any point beyond it lies within one cell (per axis) of an
// unmarked sample, hence in a cell without candidates — with a whole cell to spare for the rounding of the reference's own cell arithmetic.
// Returns `near` when no sample is marked (nothing to march).  Not for --cut (static samples need no candidates).
__device__ inline float ray_end_of_candidates(const MarchParams& a, const RayConsts& c, const uint32_t* bits2, float near) {
    const float far = c.far;
    const float rhgs = __builtin_amdgcn_rcpf(a.hgs);
    const float dts = 0.9f * a.hgs * __builtin_amdgcn_rsqf(c.dx * c.dx + c.dy * c.dy + c.dz * c.dz);
    if (!(dts > 0.0f) || !(far - near < 1e3f * dts)) return far;  // degenerate direction or an absurdly long ray: no shortcut
    float s_prev = far, s = far;
    while (true) {
        const int g0 = min(max((int)floorf((c.ox + s * c.dx - c.bmin0) * rhgs), 0), c.r0 - 1);
        const int g1 = min(max((int)floorf((c.oy + s * c.dy - c.bmin1) * rhgs), 0), c.r1 - 1);
        const int g2 = min(max((int)floorf((c.oz + s * c.dz - c.bmin2) * rhgs), 0), c.r2 - 1);
        if (cell_bit(bits2, cell_index(c, g0, g1, g2))) return s_prev;
        if (!(s > near)) return near;
        s_prev = s;
        s = fmaxf(s - dts, near);
    }
}

// ---- the two DDAs.  Same shape and the same result, but NOT the same rules at a doubtful crossing, on purpose: the cell DDA looks at every lateral neighbour
// of both cells, the region DDA at one face's pair and otherwise ends the walk at the last clear crossing.  Which element a ray restarts at, and with it the
// visited-point counts, depends on them.
struct DdaStop {
    int kind;  // 0: nothing crossed; 1: stopped at the face at parameter t, crossed on axis m; 2: nothing can happen before `far`
    float t;
    int m;
};

// The search cells the ray crosses from parameter t on, while the next one has no candidates.
__device__ inline DdaStop cell_dda(const MarchParams& a, const RayConsts& c, const uint32_t* cell_bits, const uint32_t* cell_bits2, float t) {
    const float rhgs = __builtin_amdgcn_rcpf(a.hgs);
    float xs0, ys0, zs0;
    sample_pos(a, c, false, t, xs0, ys0, zs0);
    const float q0 = (xs0 - c.bmin0) * rhgs, q1 = (ys0 - c.bmin1) * rhgs, q2 = (zs0 - c.bmin2) * rhgs;
    const float f0 = floorf(q0), f1 = floorf(q1), f2 = floorf(q2);
    const float e0 = q0 - f0, e1 = q1 - f1, e2 = q2 - f2;
    const bool sure0 = face_clear(e0) && face_clear(e1) && face_clear(e2) && fmaxf(fabsf(q0), fmaxf(fabsf(q1), fabsf(q2))) < 1e6f;
    int c0 = (int)f0, c1 = (int)f1, c2 = (int)f2;
    // the start cell has candidates, or the start lies next to a face and within one cell of candidates: the hops decide
    if (cell_outside(c, c0, c1, c2)) return {0, t, 0};
    const int cg = cell_index(c, c0, c1, c2);
    if (cell_bit(cell_bits, cg) || (!sure0 && cell_bit(cell_bits2, cg))) return {0, t, 0};
    const int st0 = c.dx > 0.0f ? 1 : -1, st1 = c.dy > 0.0f ? 1 : -1, st2 = c.dz > 0.0f ? 1 : -1;
    const bool use0 = fabsf(c.dx) > 1e-6f, use1 = fabsf(c.dy) > 1e-6f, use2 = fabsf(c.dz) > 1e-6f;
    // parameter of the next face per axis, recomputed from the cell index (no accumulation) for the axis that moved only
    float tf0 = use0 ? ((c.bmin0 + (float)(c0 + (st0 > 0)) * a.hgs) - c.ox) * c.rdx : FLT_MAX;
    float tf1 = use1 ? ((c.bmin1 + (float)(c1 + (st1 > 0)) * a.hgs) - c.oy) * c.rdy : FLT_MAX;
    float tf2 = use2 ? ((c.bmin2 + (float)(c2 + (st2 > 0)) * a.hgs) - c.oz) * c.rdz : FLT_MAX;
    int crossed = 0, m_stop = 0;
    float t_stop = t;
    for (int it = 0; it < 96; it++) {
        const int m = (tf0 <= tf1 && tf0 <= tf2) ? 0 : (tf1 <= tf2 ? 1 : 2);
        const float tx = m == 0 ? tf0 : (m == 1 ? tf1 : tf2);
        if (!(tx < c.far)) return {2, t_stop, m_stop};  // no candidates and no doubt all the way
        const float fr0 = ((c.ox + tx * c.dx) - c.bmin0) * rhgs - (float)c0, fr1 = ((c.oy + tx * c.dy) - c.bmin1) * rhgs - (float)c1,
                    fr2 = ((c.oz + tx * c.dz) - c.bmin2) * rhgs - (float)c2;
        const bool ok0 = m == 0 || face_clear(fr0), ok1 = m == 1 || face_clear(fr1), ok2 = m == 2 || face_clear(fr2);
        const bool unsafe = !(ok0 && ok1 && ok2) || !(tx > t_stop);  // next to another face, or an edge / corner (two faces at one parameter)
        const int n0 = c0 + (m == 0 ? st0 : 0), n1 = c1 + (m == 1 ? st1 : 0), n2 = c2 + (m == 2 ? st2 : 0);
        if (tx > t_stop) { t_stop = tx; m_stop = m; }
        if (cell_outside(c, n0, n1, n2)) break;
        if (cell_bit(cell_bits, cell_index(c, n0, n1, n2))) break;
        if (unsafe) {
            // the lateral neighbours the rounding could mean: one step towards every face the crossing point is close to, for the cell
            // being left and the cell being entered; every one of them must exist and be free of candidates
            const int l0 = (m == 0 || ok0) ? 0 : (fr0 < 0.5f ? -1 : 1), l1 = (m == 1 || ok1) ? 0 : (fr1 < 0.5f ? -1 : 1),
                      l2 = (m == 2 || ok2) ? 0 : (fr2 < 0.5f ? -1 : 1);
            bool blocked = !(tx > t_stop - 1e-6f * fmaxf(1.0f, fabsf(tx)));  // a face clearly BEHIND the last one: not a rounding matter
            for (int q = 1; q < 8 && !blocked; q++) {  // the non-empty subsets of the (at most two) lateral steps
                const int s0 = (q & 1) ? l0 : 0, s1 = (q & 2) ? l1 : 0, s2 = (q & 4) ? l2 : 0;
                if ((s0 | s1 | s2) == 0 || ((q & 1) && !l0) || ((q & 2) && !l1) || ((q & 4) && !l2)) continue;
                for (int side = 0; side < 2; side++) {
                    const int y0 = (side ? n0 : c0) + s0, y1 = (side ? n1 : c1) + s1, y2 = (side ? n2 : c2) + s2;
                    if (cell_outside(c, y0, y1, y2)) { blocked = true; break; }
                    if (cell_bit(cell_bits, cell_index(c, y0, y1, y2))) { blocked = true; break; }
                }
            }
            if (blocked) break;
        }
        c0 = n0; c1 = n1; c2 = n2;
        if (m == 0) tf0 = ((c.bmin0 + (float)(c0 + (st0 > 0)) * a.hgs) - c.ox) * c.rdx;
        else if (m == 1) tf1 = ((c.bmin1 + (float)(c1 + (st1 > 0)) * a.hgs) - c.oy) * c.rdy;
        else tf2 = ((c.bmin2 + (float)(c2 + (st2 > 0)) * a.hgs) - c.oz) * c.rdz;
        crossed++;
    }
    return {crossed >= 1 ? 1 : 0, t_stop, m_stop};
}

struct RegionGrid {
    const uint32_t* bits;  // LDS: bit (b2 R + b1) R + b0
    int R;                 // regions per axis = H / 8
    float lo, w, rw;       // -bound, region width 2 bound / R, its reciprocal
};
__device__ __forceinline__ bool region_set(const RegionGrid& g, int b0, int b1, int b2) { return cell_bit(g.bits, (b2 * g.R + b1) * g.R + b0); }
__device__ __forceinline__ bool region_outside(const RegionGrid& g, int b0, int b1, int b2) {
    return b0 < 0 || b1 < 0 || b2 < 0 || b0 >= g.R || b1 >= g.R || b2 >= g.R;
}
// From parameter t (a point strictly inside the volume): the last face crossed into a region without the bit before an interesting region, the volume's
// boundary or a doubt.
__device__ inline DdaStop region_dda(const RegionGrid& g, const RayConsts& c, float t) {
    // the start may lie ON (or a padding in front of) the volume's boundary — a frame's rays start where they enter the box +-(bound + 1e-3) — and the chain clamps
    // its sample positions onto +-bound: a clamp along the face normal only.  So the start's coordinates are clamped into the grid, and a lateral neighbour
    // beyond the volume does not exist — nothing can be filed there — instead of blocking the look-ahead
    const float Rf = (float)g.R;
    const float q0 = fminf(fmaxf(((c.ox + t * c.dx) - g.lo) * g.rw, 0.0f), Rf), q1 = fminf(fmaxf(((c.oy + t * c.dy) - g.lo) * g.rw, 0.0f), Rf),
                q2 = fminf(fmaxf(((c.oz + t * c.dz) - g.lo) * g.rw, 0.0f), Rf);
    if (!(q0 >= 0.0f && q1 >= 0.0f && q2 >= 0.0f)) return {0, t, 0};   // NaN
    const float f0 = fminf(floorf(q0), Rf - 1.0f), f1 = fminf(floorf(q1), Rf - 1.0f), f2 = fminf(floorf(q2), Rf - 1.0f);
    int c0 = (int)f0, c1 = (int)f1, c2 = (int)f2;
    if (region_set(g, c0, c1, c2)) return {0, t, 0};   // the common early exit: inside an interesting region
    const float e0 = q0 - f0, e1 = q1 - f1, e2 = q2 - f2;   // in [0, 1] (1: on the volume's far face)
    const int s_l0 = e0 < FACE_DOUBT_LO ? -1 : (e0 > FACE_DOUBT_HI ? 1 : 0), s_l1 = e1 < FACE_DOUBT_LO ? -1 : (e1 > FACE_DOUBT_HI ? 1 : 0),
              s_l2 = e2 < FACE_DOUBT_LO ? -1 : (e2 > FACE_DOUBT_HI ? 1 : 0);
    if (s_l0 | s_l1 | s_l2) {   // a start next to a face: the regions it could be taken for
        for (int q = 1; q < 8; q++) {
            if (((q & 1) && !s_l0) || ((q & 2) && !s_l1) || ((q & 4) && !s_l2)) continue;
            const int y0 = c0 + ((q & 1) ? s_l0 : 0), y1 = c1 + ((q & 2) ? s_l1 : 0), y2 = c2 + ((q & 4) ? s_l2 : 0);
            if (region_outside(g, y0, y1, y2)) continue;   // beyond the volume
            if (region_set(g, y0, y1, y2)) return {0, t, 0};
        }
    }
    const int st0 = c.dx > 0.0f ? 1 : -1, st1 = c.dy > 0.0f ? 1 : -1, st2 = c.dz > 0.0f ? 1 : -1;
    const bool use0 = fabsf(c.dx) > 1e-6f, use1 = fabsf(c.dy) > 1e-6f, use2 = fabsf(c.dz) > 1e-6f;
    float tf0 = use0 ? ((g.lo + (float)(c0 + (st0 > 0)) * g.w) - c.ox) * c.rdx : FLT_MAX;
    float tf1 = use1 ? ((g.lo + (float)(c1 + (st1 > 0)) * g.w) - c.oy) * c.rdy : FLT_MAX;
    float tf2 = use2 ? ((g.lo + (float)(c2 + (st2 > 0)) * g.w) - c.oz) * c.rdz : FLT_MAX;
    // where a crossing lies between the faces of another axis, from the face parameters alone: u = (tf_axis - tx) |d_axis| / w is the way left to that
    // axis's next face in region widths (0: on it, 1: on the one behind).  An axis the ray runs along keeps its start position between its faces.
    const float k0 = fabsf(c.dx) * g.rw, k1 = fabsf(c.dy) * g.rw, k2 = fabsf(c.dz) * g.rw;
    const float u_fix0 = st0 > 0 ? 1.0f - e0 : e0, u_fix1 = st1 > 0 ? 1.0f - e1 : e1, u_fix2 = st2 > 0 ? 1.0f - e2 : e2;
    int crossed = 0;
    float t_stop = t;
    int m_stop = 0;
    for (int it = 0; it < 3 * g.R + 3; it++) {
        const int m = (tf0 <= tf1 && tf0 <= tf2) ? 0 : (tf1 <= tf2 ? 1 : 2);
        const float tx = m == 0 ? tf0 : (m == 1 ? tf1 : tf2);
        if (!(tx < c.far)) return {2, t_stop, m_stop};
        const float u0 = use0 ? (tf0 - tx) * k0 : u_fix0, u1 = use1 ? (tf1 - tx) * k1 : u_fix1, u2 = use2 ? (tf2 - tx) * k2 : u_fix2;
        const bool ok0 = m == 0 || face_clear(u0), ok1 = m == 1 || face_clear(u1), ok2 = m == 2 || face_clear(u2);
        // a crossing within 2e-3 region widths of another face: the reference's float arithmetic may file the elements around it under the lateral neighbour
        // across that face — of the region being left or of the one being entered.  ONE such face: those two regions are looked at, and the walk goes on if
        // neither has the bit.  Two (an edge or a corner, or two faces at one parameter): the walk ends at the last crossing that was clear — between two clear
        // crossings the ray's distance to the lateral faces lies between its values at the two — and the exact hops take the ray past the doubtful one.
        // (The first version ran a 14-way neighbour loop here, which one lane in a hundred takes and its whole wave waits for: 26 of the first look-ahead's 62 us
        // on the trex option set; ending the walk at EVERY doubtful crossing instead cost more than that in the extra look-aheads of the rays that meet nothing.)
        const int n0 = c0 + (m == 0 ? st0 : 0), n1 = c1 + (m == 1 ? st1 : 0), n2 = c2 + (m == 2 ? st2 : 0);
        if (!(tx > t_stop)) break;
        if (!(ok0 && ok1 && ok2)) {
            const int l0 = (m == 0 || ok0) ? 0 : (u0 < 0.5f ? st0 : -st0), l1 = (m == 1 || ok1) ? 0 : (u1 < 0.5f ? st1 : -st1), l2 = (m == 2 || ok2) ? 0 : (u2 < 0.5f ? st2 : -st2);
            if ((l0 != 0) + (l1 != 0) + (l2 != 0) != 1) break;
            const int a0 = c0 + l0, a1 = c1 + l1, a2 = c2 + l2, b0 = n0 + l0, b1 = n1 + l1, b2 = n2 + l2;
            if (region_outside(g, a0, a1, a2) || region_outside(g, b0, b1, b2)) break;
            if (region_set(g, a0, a1, a2) || region_set(g, b0, b1, b2)) break;
        }
        t_stop = tx;
        m_stop = m;
        if (region_outside(g, n0, n1, n2)) break;   // the volume's boundary: points beyond are clamped onto it
        if (region_set(g, n0, n1, n2)) break;
        c0 = n0; c1 = n1; c2 = n2;
        if (m == 0) tf0 = ((g.lo + (float)(c0 + (st0 > 0)) * g.w) - c.ox) * c.rdx;
        else if (m == 1) tf1 = ((g.lo + (float)(c1 + (st1 > 0)) * g.w) - c.oy) * c.rdy;
        else tf2 = ((g.lo + (float)(c2 + (st2 > 0)) * g.w) - c.oz) * c.rdz;
        crossed++;
    }
    return {crossed >= 1 ? 1 : 0, t_stop, m_stop};
}

// ---- the restart search: the last certainly-visited element more than a face margin before the DDA's stopping face.
// Fixed step: the elements in front of the face are t + k * Dq.  Returns the element to go on from, t itself when there is none within 32 tries or the face
// lies in another binade.
__device__ __forceinline__ float restart_on_lattice(const MarchParams& a, const RayConsts& c, float D, float t, float t_stop, int m_stop) {
    const Binade bn = binade_of<1>(t, D);
    const float kcap = lattice_k_cap(bn, t);
    float rd_stop;
    const float target = t_stop - face_margin(c, m_stop, t, rd_stop);
    if (bn.ok && target > t && target < bn.top && rd_stop < RD_MAX) {
        float kf = fminf(floorf((target - t) * bn.rDq), kcap);
        if (kf >= 1.0f && t + kf * bn.Dq > target) kf -= 1.0f;
        for (int tries = 0; tries < 32 && kf >= 2.0f; tries++, kf -= 1.0f) {
            const float e = t + kf * bn.Dq, p = t + (kf - 1.0f) * bn.Dq;  // exact: both inside the binade, k below the exactness cap
            float x, y, z;
            sample_pos(a, c, false, p, x, y, z);
            if (certainly_visited(c, p, e, t, x, y, z, a.bound, c.rbound)) return e;  // bound <= 1, one cascade: mip_bound = fminf(2^0, bound) = bound
        }
    }
    return t;
}
// Any step: walk the t-sequence (the chain's own step expression) from t to the zone [zone, target), then look for the LAST pair (p, e) of consecutive elements
// in it that restarts the chain, p at least w_t (one top-level voxel diagonal) into a run of elements on one mip level.  Returns e, or -1.
__device__ __forceinline__ float restart_on_sequence(const MarchParams& a, const RayConsts& c, bool one_cascade, float t, float zone, float target, float w_t) {
    float T = t;
    while (true) {   // four elements per exit test (the walk is a large part of a long look-ahead: up to ~150 elements)
        const float T1 = T + dtf(a, c, T);
        const float T2 = T1 + dtf(a, c, T1);
        const float T3 = T2 + dtf(a, c, T2);
        const float T4 = T3 + dtf(a, c, T3);
        if (T4 < zone) { T = T4; continue; }
        T = T3 < zone ? T3 : (T2 < zone ? T2 : (T1 < zone ? T1 : T));   // the last element in front of the zone
        break;
    }
    float best = -1.0f, run_start = FLT_MAX;
    int run_level = -1;
    for (int it = 0; it < 512; it++) {   // (w_t / dt_min elements at most: a few dozen)
        const float pT = T, eT = T + dtf(a, c, T);
        if (!(eT < target)) break;
        float x, y, z;
        sample_pos(a, c, true, pT, x, y, z);
        const int level = mip_level(a, c, one_cascade, x, y, z, pT);
        if (level != run_level) { run_level = level; run_start = pT; }
        if (run_start <= pT - w_t) {
            float mip_bound, mip_rbound;
            mip_scale(a, c, level, mip_bound, mip_rbound);
            if (certainly_visited(c, pT, eT, pT, x, y, z, mip_bound, mip_rbound)) best = eT;
        }
        T = eT;
    }
    return best;
}

// One region look-ahead from t (--cut).  Returns false when nothing interesting lies before `far` (the chain walks there and emits nothing); otherwise t has
// been moved to a visited element in a region without the bit — the exact hops go on from there — or left alone.
__device__ __forceinline__ bool region_look_ahead(const MarchParams& a, const RayConsts& c, const RegionGrid& maps, bool one_cascade, float w_t, float& t,
                                                  int& retry_hops) {
    const float px = c.ox + t * c.dx, py = c.oy + t * c.dy, pz = c.oz + t * c.dz;
    // inside the volume, or just in front of it: a frame's rays start on the box +-(bound + 1e-3) (renderer.py:782-791 pads the box), and the chain clamps its
    // sample positions onto +-bound — which region_dda's clamped start coordinates reproduce.  (Rounds of the first version began with a look-ahead that
    // this test refused for every ray: the real first one came six hops later.)
    const float b_in = a.bound + 2e-3f;
    if (!(fabsf(px) <= b_in && fabsf(py) <= b_in && fabsf(pz) <= b_in)) return true;
    // the map of the ray's minimum mip level from here on: level = max(from the position, from dt) >= mip_from_dt(dt(t)), and dt does not fall along the ray —
    // on the trex option set dt puts every point on level 1, and what is occupied on level 0 only cannot be met
    const int lv_min = one_cascade ? 0 : mip_from_dt(dtf(a, c, t), c.Hf, c.Cf);
    RegionGrid rg = maps;  // (`maps.bits`: level 0's map, the others behind it)
    rg.bits += (size_t)lv_min * (size_t)((rg.R * rg.R * rg.R) >> 5);
    const DdaStop s = region_dda(rg, c, t);
    if (s.kind == 2) return false;
    float rd_stop;
    const float target = s.t - face_margin(c, s.m, s.t, rd_stop);
    // the zone in front of `target` in which the restart pair is looked for: a voxel diagonal of same-level elements behind p, then p and e
    const float zone_len = 1.1f * w_t + 3.0f * dtf(a, c, target);
    if (s.kind == 1 && rd_stop < RD_MAX && target - zone_len - w_t > t) {
        const float best = restart_on_sequence(a, c, one_cascade, t, target - zone_len, target, w_t);
        if (best > t) t = best;
        else retry_hops = min(retry_hops * 4, 64);   // (no pair: a mip level change or a grazing ray — do not pay for the same look-ahead every few hops)
    }
    return true;
}

struct SkipMaps {  // what k_march_skip hands over (each may be null / 0: that look-ahead or shortcut is off)
    const uint32_t* cell_bits;     // LDS: bit c set <=> search cell c has candidates
    const uint32_t* cell_bits2;    // LDS: cells within one cell of one with candidates — with cell_bits and without --cut: the cell look-ahead is on
    const uint32_t* grid_regions;  // LDS: --cut, the region maps, one per minimum mip level
    int regions_R;                 // regions per axis
    int hop_budget;                // > 0 (with the cell look-ahead): hops before the ray is handed on
};

// `c`: the ray's constants (ray_consts), c.far the end the caller wants (ray_end_of_candidates where there is one).  n_iter_out: the hops walked.
__device__ inline float skip_empty_cells(const MarchParams& a, const March2Tables& tb, const RayConsts& c, const SkipMaps& mp, int index, float noise,
                                         unsigned* n_iter_out) {
    *n_iter_out = 0;
    RayState st;
    if (!ray_start(a, c, index, noise, nullptr, st)) return st.t;
    float t = st.t;
    const bool cut = a.cut != 0, one_cascade = a.C == 1, fixed = a.dt_gamma == 0.0f;
    const float D = clampf(0.0f, c.dt_min, c.dt_max);
    LatticeWalk lw;
    unsigned n_iter = 0;
    if (!cut && mp.cell_bits) {
        // The common case (no --cut, emptiness bits in LDS) with as few branches as the semantics allow: the kernel is issue-bound (its busy
        // waves share a third of the SIMDs) and the general loop below costs ~25 exec-mask branches per hop.
        if (mp.cell_bits2 && fixed && one_cascade && a.bound <= 1.0f) {
            const DdaStop s = cell_dda(a, c, mp.cell_bits, mp.cell_bits2, t);
            if (s.kind == 2) return c.far;
            if (s.kind == 1) t = restart_on_lattice(a, c, D, t, s.t, s.m);
        }
        while (true) {
            float x, y, z;
            int g0, g1, g2;
            sample_pos(a, c, false, t, x, y, z);
            cell_coords(a, c, x, y, z, g0, g1, g2);
            const bool inside = !cell_outside(c, g0, g1, g2);
            const bool has = cell_bit(mp.cell_bits, inside ? cell_index(c, g0, g1, g2) : 0);
            if (!inside || has) break;  // outside the hash (the windowed march raises the error flag) or candidates: hand over
            if (mp.hop_budget > 0 && (int)n_iter >= mp.hop_budget) break;  // a straggler: the windowed march goes on from this (visited) element
            float mip_bound, mip_rbound;
            mip_scale(a, c, mip_level(a, c, one_cascade, x, y, z, t), mip_bound, mip_rbound);
            const VoxelHop v = voxel_hop(c, x, y, z, mip_bound, mip_rbound);
            n_iter++;
            t = advance_past(a, c, fixed, D, lw, t, hop_target(t, v));
            if (!(t < c.far)) break;
        }
        *n_iter_out = n_iter;
        return t;
    }
    // The general loop: --cut (with the region look-ahead where the caller built the maps: bound == 2^(C - 1), so level l's voxels are 2^(l + 1) / H wide and a
    // region is 8^3 voxels of level C - 1), or no bits in LDS (the candidate ranges are read from global memory, once per cell).
    const bool regions_on = cut && mp.grid_regions != nullptr && mp.regions_R > 0;
    const RegionGrid rg{mp.grid_regions, mp.regions_R, -a.bound, 2.0f * a.bound / (float)max(mp.regions_R, 1), (float)max(mp.regions_R, 1) / (2.0f * a.bound)};
    const float rnorm = __builtin_amdgcn_rsqf(c.dx * c.dx + c.dy * c.dy + c.dz * c.dz);
    const float w_t = 1.7320508f * 2.0f * a.bound * c.rH * rnorm * 1.02f;   // one top-level voxel diagonal in units of t (+ 2 %)
    int hops_since_try = 0, retry_hops = PN_REGION_RETRY_HOPS;
    bool try_regions = regions_on && w_t > 0.0f && w_t < 1e3f;
    float cb[6] = {0, 0, 0, 0, 0, 0};
    if (cut)
        for (int i = 0; i < 6; i++) cb[i] = a.cut_bounds[i];
    int cell_id = -1;
    while (t < c.far) {
        if (try_regions) {
            try_regions = false;
            hops_since_try = 0;
            if (!region_look_ahead(a, c, rg, one_cascade, w_t, t, retry_hops)) { *n_iter_out = n_iter; return c.far; }
        }
        float x, y, z;
        sample_pos(a, c, cut, t, x, y, z);
        const bool searched = !cut || inside_cut_box(cb, x, y, z);
        if (searched) {
            int g0, g1, g2;
            cell_coords(a, c, x, y, z, g0, g1, g2);
            if (cell_outside(c, g0, g1, g2)) break;  // the windowed march raises the error flag
            const int gid = cell_index(c, g0, g1, g2);
            if (gid != cell_id) {
                const bool has = mp.cell_bits ? cell_bit(mp.cell_bits, gid) : tb.nb_rng[gid].x != tb.nb_rng[gid].y;
                if (has) break;  // candidates: hand over
                cell_id = gid;
            }
        }
        // found == false (or a static sample in an empty voxel): un-warped voxel skip (raymarching.cu:1386-1428)
        const int level = mip_level(a, c, one_cascade, x, y, z, t);
        float mip_bound, mip_rbound;
        mip_scale(a, c, level, mip_bound, mip_rbound);
        const VoxelHop v = voxel_hop(c, x, y, z, mip_bound, mip_rbound);
        if (!searched) {  // static sample: emitted when its voxel is occupied -> hand over to the windowed march at this element
            const uint32_t vox = (uint32_t)(level * c.H3 + (float)morton3D(v.nx, v.ny, v.nz));
            if (a.grid[vox / 8] & (1 << (vox % 8))) break;
        }
        n_iter++;
        if (regions_on && ++hops_since_try >= retry_hops) try_regions = true;   // past an interesting region without an event: look ahead again
        t = advance_past(a, c, fixed, D, lw, t, hop_target(t, v));
    }
    *n_iter_out = n_iter;
    return t;
}

}  // namespace pnm3
