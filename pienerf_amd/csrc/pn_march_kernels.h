// The march kernels of the render unit and their launchers: the skip pre-pass, the per-ray march in its two passes, the frame form of the static march.
// Part of the render unit (included by pn_render_ops.hip only).
#pragma once
#include "pn_march_static.h"
#include "pn_march_skip.h"
#include "pn_march_window.h"
#include "pn_render_records.h"

// One lane per ray slot: fast-forward over the leading run of IP-free search cells (pn_march_skip.h).
__global__ void __launch_bounds__(256) k_march_skip(pnm::MarchParams a, pnm2::March2Tables tb, MarchIO io) {
    extern __shared__ uint32_t bits_lds[];
    uint32_t n_alive = io.n_alive;
    if (io.trip) n_alive = (uint32_t)io.trip->n_alive;
    const uint32_t n = threadIdx.x + blockIdx.x * blockDim.x;
    const uint32_t *cell_bits = nullptr, *cell_bits2 = nullptr;
    if (io.cell_bits_words > 0) {  // uniform
        const int n_grid = a.resolution[0] * a.resolution[1] * a.resolution[2];
        const int words = min((n_grid + 31) >> 5, io.cell_bits_words);
        for (int w = threadIdx.x; w < words; w += blockDim.x) bits_lds[w] = io.cell_bits[w];
        cell_bits = bits_lds;
        if (io.cell_bits2 && io.fars_eff && !a.cut) {
            for (int w = threadIdx.x; w < words; w += blockDim.x) bits_lds[io.cell_bits_words + w] = io.cell_bits2[w];
            cell_bits2 = bits_lds + io.cell_bits_words;
        }
        __syncthreads();
    }
    const uint32_t* grid_regions = nullptr;
    if (io.grid_regions_words > 0) {  // uniform; behind the cell maps (the launch's dynamic LDS counts it in)
        uint32_t* gb = bits_lds + (io.cell_bits_words > 0 ? io.cell_bits_words * ((io.cell_bits2 && io.fars_eff && !a.cut) ? 2 : 1) : 0);
        for (int w = threadIdx.x; w < io.grid_regions_words; w += blockDim.x) gb[w] = io.grid_regions[w];
        grid_regions = gb;
        __syncthreads();
    }
    bool work = false;
    if (n < n_alive) {
        unsigned n_iter = 0;
        const int index = io.rays_alive[n];
        pnm3::RayConsts c;
        pnm3::ray_consts(a, index, c);
        if (cell_bits2) {  // shorten the ray to where it can still find candidates (the end is taken as it comes: near >= the driver's min_near > 0)
            const float near = a.rays_t[index];
            if (near < c.far) c.far = pnm3::ray_end_of_candidates(a, c, cell_bits2, near);
            io.fars_eff[index] = c.far;
        }
        const bool dda = io.dda_start && cell_bits2;
        const pnm3::SkipMaps maps{cell_bits, dda ? cell_bits2 : nullptr, grid_regions, io.grid_regions_R, dda ? io.hop_budget : 0};
        const float t = pnm3::skip_empty_cells(a, tb, c, maps, index, io.noises ? io.noises[n] : 0.0f, &n_iter);
        io.t_resume[n] = t;
        if (!PN_DBG_PHASES_ON && a.stats && n_iter) atomicAdd(a.stats, (unsigned long long)n_iter);
        work = t < c.far;
        if (io.active && !work) {  // nothing left to march: k_march will not visit the slot, so its (single, n_step == 1) sample slot is ended here
            const uint32_t n_step = (uint32_t)io.trip->n_step;
            float* dl = io.deltas + (size_t)n * n_step * 2;
            for (uint32_t s2 = 0; s2 < n_step; s2++) { dl[2 * s2] = 0.0f; dl[2 * s2 + 1] = 0.0f; }
        }
    }
    if (io.active) {  // wave-aggregated append to this wave's segment (order is irrelevant: every listed slot is processed independently)
        const unsigned long long m = __ballot(work);
        const int lane = threadIdx.x & 63;
        const int seg = (int)((n >> 6) % PN_SEGS);
        int base = 0;
        if (lane == 0 && m) base = atomicAdd(io.active_counts + seg * PN_SEG_STRIDE, (int)__popcll(m));
        base = __shfl(base, 0);
        if (work) io.active[(size_t)seg * io.active_seg_cap + base + (int)__popcll(m & ((1ull << lane) - 1ull))] = (int)n;
    }
}

// ---- the per-ray march (pn_march_window.h): pass 1 = k_march (8 lanes per ray, bounded number of rounds), pass 2 = k_march_tail
// (one wave per ray that pass 1 left unfinished).

// waves per SIMD the march kernels ask for.  What really sets their occupancy is LDS: 12 KB of staging per wave (PN_STAGE_CAP) = three
// workgroups per CU, and the compiler then takes the registers three waves per SIMD leave it (~160 VGPRs, no spills).  One wave per SIMD is
// only 15 % slower for the march alone (a wave is a chain of dependent instructions and round trips), but what a march wave holds while it
// waits is what the other render lanes and the simulator cannot use (launch structure)
#ifndef PN_MARCH_WAVES
#define PN_MARCH_WAVES 4
#endif

// G = 8: 8 lanes per ray (each lane one point of the ray's t-sequence per round), 32 rays per 256-thread block.
// G = 1: ONE lane per ray, 256 rays per block — every evaluated point is a visited one (no speculation: a quarter of the VALU work per visited point of
// the windows, whose lanes evaluate 4.6 elements per voxel hop), at one visited point per round (the windows: ~14).  The throughput form of a frame's
// first trip (pn_render_opts.throughput): the wave-per-ray tail pass that the pipelined step is bound by only gets the rays that outlast the budget.
template <int K, bool MULTI, int G>
__global__ void __launch_bounds__(256, PN_MARCH_WAVES) k_march(pnm::MarchParams a, pnm2::March2Tables tb, MarchIO io) {
    uint32_t n_alive = io.n_alive, n_step_trip = io.n_step;
    bool dense = false;
    if (io.trip) { n_alive = (uint32_t)io.trip->n_alive; n_step_trip = (uint32_t)io.trip->n_step; dense = trip_is_dense(io.trip); }
    static_assert(G == 8 || G == 1, "lanes per ray");
    constexpr uint32_t RB = 256u / G;  // rays per chunk: a workgroup's share per step of its loop
    const int lane = threadIdx.x & 63, sub = lane & (G - 1), gbase = lane & ~(G - 1);
    const int budget = io.tail ? io.max_rounds : 0x7fffffff;
    __shared__ float4 stage_mem[4][PN_STAGE_CAP];
    float4* stage = stage_mem[threadIdx.x >> 6];
    // 32-ray chunks are dealt round-robin to a bounded grid: in frame mode the alive count is only known on the device, and a
    // grid sized for all N rays would push ~20 000 mostly empty workgroups through the dispatcher on every trip.  With an active list
    // (trip 0) workgroup b walks segment b % PN_SEGS of it; either way `seg` names the segment this workgroup's own appends go to.
    const uint32_t unit = blockIdx.x, n_units = gridDim.x;
    const uint32_t act_seg = unit % PN_SEGS;
    const uint32_t n_work = io.active ? (uint32_t)seg_count(io.active_counts, (int)act_seg) : n_alive;
    const uint32_t k0 = io.active ? unit / PN_SEGS : unit, kstep = io.active ? (uint32_t)seg_workers((int)n_units, (int)act_seg) : n_units;
    PN_PHASE_DECL(pk);
    for (uint32_t chunk = k0; chunk * RB < n_work; chunk += kstep) {
        const uint32_t seg = io.active ? act_seg : chunk % PN_SEGS;
        const uint32_t i_work = chunk * RB + threadIdx.x / G;
        const uint32_t n = io.active ? (i_work < n_work ? (uint32_t)io.active[(size_t)act_seg * io.active_seg_cap + i_work] : 0xffffffffu) : i_work;
        uint32_t emitted = 0;
        bool deferred = false, have = false;
        float* dl = nullptr;
        pnm3::RayConsts c;
        pnm3::RayState st{0.f, 0.f, 0u};
        uint32_t n_step = n_step_trip, slot0 = 0;  // per ray with ray groups
        if (n < n_alive) {
            const int index = io.rays_alive[n];
            const float noise = io.noises ? io.noises[n] : 0.0f;
            ray_slots(io.groups, io.group_rays, index, n, n_step, slot0);
            dl = io.deltas + (size_t)slot0 * 2;
            pnm3::ray_consts(a, index, c);
            have = pnm3::ray_start(a, c, index, noise, io.t_resume ? io.t_resume + n : nullptr, st);
        }
        PN_PHASE(pk, 0);
        // all 64 lanes enter (the round loop inside is wave-uniform, pn_march_window.h); lanes without a ray idle through it
        const bool done = pnm3::march_window<K, MULTI, G>(a, tb, c, n_step, sub, gbase, lane, stage, io.xyzs + (size_t)slot0 * 3,
                                                          io.dirs + (size_t)slot0 * 3, dl, st, budget, have PN_PHASE_PASS);
        if (n < n_alive) {
            deferred = have && !done;  // still marching after the round budget: continue with a whole wave (k_march_tail)
            emitted = deferred ? 0u : st.step;  // a deferred ray's samples are listed by the tail pass
            if (!PN_DBG_PHASES_ON && a.stats && sub == 0 && emitted) atomicAdd(a.stats + 3, (unsigned long long)emitted);
        }
        if (io.tail) {  // one counter update per wave and class for all its deferred rays
            // class: more than three 64-element windows still to go (longest-first start order shortens the tail pass's critical path)
            const bool is_long = deferred && (c.far - st.t) > 192.0f * pnm3::dtf(a, c, st.t);
            const unsigned long long dm = __ballot(deferred && sub == 0), lm = __ballot(is_long && sub == 0), sm = dm & ~lm;
            if (dm) {
                int posl = 0, poss = 0;
                if (lane == 0 && lm) posl = atomicAdd(io.tail_counts + seg * PN_SEG_STRIDE, (int)__popcll(lm));
                if (lane == 0 && sm) poss = atomicAdd(io.tail_back + seg * PN_SEG_STRIDE, (int)__popcll(sm));
                posl = __shfl(posl, 0);
                poss = __shfl(poss, 0);
                if (deferred && sub < 4) {  // lanes 0..3 of the group write one 16-byte part each (G == 1: the lane writes all four)
                    const unsigned long long below = (1ull << gbase) - 1ull;
                    const int slot = is_long ? posl + (int)__popcll(lm & below) : io.tail_seg_cap - 1 - (poss + (int)__popcll(sm & below));
                    float4* te = reinterpret_cast<float4*>(io.tail + (size_t)seg * io.tail_seg_cap + slot);
#pragma unroll
                    for (int part_i = (G == 1 ? 0 : sub); part_i < (G == 1 ? 4 : sub + 1); part_i++) {
                        float4 part;
                        if (part_i == 0) part = make_float4(__int_as_float((int)n), st.t, st.last_t, __int_as_float((int)st.step));
                        else if (part_i == 1) part = make_float4(c.ox, c.oy, c.oz, c.dx);
                        else if (part_i == 2) part = make_float4(c.dy, c.dz, c.rdx, c.rdy);
                        else part = make_float4(c.rdz, c.far, __int_as_float((int)slot0), __int_as_float((int)n_step));
                        te[part_i] = part;
                    }
                }
            }
        }
        if (io.trip) {
            // slots the ray did not fill end it in composite (delta == 0); the op-level wrapper zero-fills instead (raymarching.py:415-417)
            if (dl && !deferred)
                for (uint32_t s = emitted + sub; s < n_step; s += G) { dl[2 * s] = 0.0f; dl[2 * s + 1] = 0.0f; }
            if (dense) {
                if (dl && !deferred) {
                    float* X = io.xyzs + (size_t)slot0 * 3;
                    float* Dd = io.dirs + (size_t)slot0 * 3;
                    for (uint32_t s = emitted + sub; s < n_step; s += G) { X[3 * s] = X[3 * s + 1] = X[3 * s + 2] = 0.0f; Dd[3 * s] = Dd[3 * s + 1] = Dd[3 * s + 2] = 0.0f; }
                    for (uint32_t s = sub; s < n_step; s += G) io.list[slot0 + s] = (int)(slot0 + s);
                }
                int v = (sub == 0 && dl && !deferred) ? (int)emitted : 0;  // one counter update per wave
                if (G == 1) { v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4); }
                v += __shfl_xor(v, 8); v += __shfl_xor(v, 16); v += __shfl_xor(v, 32);
                if (lane == 0 && v) atomicAdd(io.emit_parts + seg * PN_SEG_STRIDE, v);
            } else {
            // wave-aggregated append of this wave's valid sample slots (one atomic per wave)
            int inc = (sub == 0) ? (int)emitted : 0;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int u = __shfl_up(inc, o);
                if (lane >= o) inc += u;
            }
            const int total = __shfl(inc, 63);
            int base = 0;
            if (lane == 63 && total > 0) base = atomicAdd(io.samp_counts + seg * PN_SEG_STRIDE, total);
            base = __shfl(base, 63);
            const int first = base + __shfl(inc, gbase) - (int)emitted;  // exclusive prefix of this group's first lane
            int* seg_list = io.list_seg + (size_t)seg * io.list_seg_cap;
            for (uint32_t s = sub; s < emitted; s += G) seg_list[first + s] = (int)(slot0 + s);
            }
        }
        PN_PHASE(pk, 5);
    }
    PN_PHASE_FLUSH(pk, a.stats, 0, lane);
}

// One wave per unfinished ray: windows of 64 sequence elements until the ray is done for this trip.
template <int K, bool MULTI>
__global__ void __launch_bounds__(256, PN_MARCH_WAVES) k_march_tail(pnm::MarchParams a, pnm2::March2Tables tb, MarchIO io) {
    bool dense = false;
    if (io.trip) dense = trip_is_dense(io.trip);
    const int lane = threadIdx.x & 63;
    const int gw = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6), n_waves = (int)gridDim.x * 4;
    const int seg = gw % PN_SEGS;  // this wave's segment of the tail list; its own appends go to the same segment of the sample list
    const int n_long = seg_count(io.tail_counts, seg), total = n_long + seg_count(io.tail_back, seg);
    __shared__ float4 stage_mem[4][PN_STAGE_CAP];
    float4* stage = stage_mem[threadIdx.x >> 6];
    PN_PHASE_DECL(pk);
    // the rays of a segment are handed out one at a time to the waves that serve it: their lengths differ by an order of magnitude (1 to 8
    // windows), and with a fixed assignment the wave that drew several long ones set the kernel's duration
    (void)n_waves;
    for (;;) {
        int e = 0;
        if (lane == 0) e = atomicAdd(io.tail_cursors + seg * PN_SEG_STRIDE, 1);
        e = __builtin_amdgcn_readfirstlane(e);
        if (e >= total) break;
        const TailEntry te = io.tail[(size_t)seg * io.tail_seg_cap + (e < n_long ? e : io.tail_seg_cap - 1 - (e - n_long))];
        const uint32_t slot0 = (uint32_t)te.slot0, n_step = (uint32_t)te.n_step;
        float* dl = io.deltas + (size_t)slot0 * 2;
        pnm3::RayConsts c;
        c.ox = te.ox; c.oy = te.oy; c.oz = te.oz; c.dx = te.dx; c.dy = te.dy; c.dz = te.dz; c.rdx = te.rdx; c.rdy = te.rdy; c.rdz = te.rdz; c.far = te.far;
        pnm3::frame_consts(a, c);
        pnm3::RayState st{te.t, te.last_t, (uint32_t)te.step};
        PN_PHASE(pk, 0);
        pnm3::march_window<K, MULTI, 64>(a, tb, c, n_step, lane, 0, lane, stage, io.xyzs + (size_t)slot0 * 3, io.dirs + (size_t)slot0 * 3,
                                         dl, st, 0x7fffffff, true PN_PHASE_PASS);
        const uint32_t emitted = st.step;
        if (!PN_DBG_PHASES_ON && a.stats && lane == 0 && emitted) atomicAdd(a.stats + 3, (unsigned long long)emitted);
        if (io.trip) {
            for (uint32_t s = emitted + lane; s < n_step; s += 64) { dl[2 * s] = 0.0f; dl[2 * s + 1] = 0.0f; }
            if (dense) {
                float* X = io.xyzs + (size_t)slot0 * 3;
                float* Dd = io.dirs + (size_t)slot0 * 3;
                for (uint32_t s = emitted + lane; s < n_step; s += 64) { X[3 * s] = X[3 * s + 1] = X[3 * s + 2] = 0.0f; Dd[3 * s] = Dd[3 * s + 1] = Dd[3 * s + 2] = 0.0f; }
                for (uint32_t s = lane; s < n_step; s += 64) io.list[slot0 + s] = (int)(slot0 + s);
                if (lane == 0 && emitted) atomicAdd(io.emit_parts + seg * PN_SEG_STRIDE, (int)emitted);
            } else {
                int base = 0;
                if (lane == 0 && emitted > 0) base = atomicAdd(io.samp_counts + seg * PN_SEG_STRIDE, (int)emitted);
                base = __shfl(base, 0);
                int* seg_list = io.list_seg + (size_t)seg * io.list_seg_cap;
                for (uint32_t s = lane; s < emitted; s += 64) seg_list[base + s] = (int)(slot0 + s);
            }
        }
        PN_PHASE(pk, 5);
    }
    PN_PHASE_FLUSH(pk, a.stats, 6, lane);
}

template <int K, bool MULTI>
static void launch_march_km(uint32_t blocks, uint32_t tail_blocks, hipStream_t st, const pnm::MarchParams& a, const pnm2::March2Tables& tb, const MarchIO& io) {
    if (io.lane_per_ray) k_march<K, MULTI, 1><<<blocks, 256, 0, st>>>(a, tb, io);
    else k_march<K, MULTI, 8><<<blocks, 256, 0, st>>>(a, tb, io);
    if (io.tail) k_march_tail<K, MULTI><<<tail_blocks, 256, 0, st>>>(a, tb, io);
}

// pass 1 over `blocks` workgroups, then (io.tail != nullptr) the tail pass over `tail_blocks`
static void launch_march(int K, uint32_t blocks, uint32_t tail_blocks, hipStream_t st, const pnm::MarchParams& a, const pnm2::March2Tables& tb,
                         const MarchIO& io) {
    const bool multi = a.max_iter_num > 1;
    if (K == 1) { if (multi) launch_march_km<1, true>(blocks, tail_blocks, st, a, tb, io); else launch_march_km<1, false>(blocks, tail_blocks, st, a, tb, io); }
    else if (K == 2) { if (multi) launch_march_km<2, true>(blocks, tail_blocks, st, a, tb, io); else launch_march_km<2, false>(blocks, tail_blocks, st, a, tb, io); }
    else { if (multi) launch_march_km<3, true>(blocks, tail_blocks, st, a, tb, io); else launch_march_km<3, false>(blocks, tail_blocks, st, a, tb, io); }
}

// Rounds of 8 sequence elements a ray gets in k_march before it is handed to the wave-per-ray tail pass.
static int g_skip_dda_override = -1;    // pn_march_set_skip_dda (tests): 0 / 1 replace the default, -1: default (1)
static int g_tail_rounds_override = 0;  // pn_march_set_tail_rounds (tests): > 0 replaces the default below
// Defaults measured on the chair once the append lists were segmented (k_march + tail per trip, us): trip 0 (every ray looks for its first sample)
// 232 / 201 / 210 / 211 for 1 / 2 / 3 / 4 rounds; later trips (alive rays, 8 samples each: most are done after one window) 70 / 76 / 78 / 79.
static uint32_t march_tail_rounds(int trip = -1) {
    if (g_tail_rounds_override > 0) return (uint32_t)g_tail_rounds_override;
    return trip < 0 ? 4u : (trip == 0 ? 2u : 1u);
}

static pnm::MarchParams make_march_params(const int* pig_cnt, const int* pig_bgn, const int* pig_idx, int n_vtx, int n_grid, const float* p_def,
                                          const float* p_ori, const float* F_IP, const float* dF_IP, int max_iter_num, const float* bbmin,
                                          const float* bbmax, float hgs, const int* resolution, int num_seek_IP, float IP_dx, int cut,
                                          const float* cut_bounds, const float* rays_t, const float* rays_o, const float* rays_d, float bound,
                                          float dt_gamma, uint32_t max_steps, uint32_t C, uint32_t H, const uint8_t* grid, const float* fars,
                                          int* err_flag) {
    pnm::MarchParams a;
    a.pig_cnt = pig_cnt; a.pig_bgn = pig_bgn; a.pig_idx = pig_idx; a.n_vtx = n_vtx; a.n_grid = n_grid;
    a.p_ori = p_ori; a.p_def = p_def; a.F_IP = F_IP; a.dF_IP = dF_IP; a.max_iter_num = max_iter_num;
    a.bbmin = bbmin; a.bbmax = bbmax; a.hgs = hgs; a.resolution = resolution; a.num_seek_IP = num_seek_IP; a.IP_dx = IP_dx;
    a.cut = cut; a.cut_bounds = cut_bounds; a.rays_t = rays_t; a.rays_o = rays_o; a.rays_d = rays_d;
    a.bound = bound; a.dt_gamma = dt_gamma; a.max_steps = max_steps; a.C = C; a.H = H; a.grid = grid; a.fars = fars; a.err_flag = err_flag;
    a.stats = nullptr;
    return a;
}

// Frame-driver form of the static march (pn_render_static): counts come from the trip record, 256-ray chunks are dealt round-robin to a
// bounded grid, unfilled slots are ended (delta = 0) and the valid sample slots are appended to `list` (one atomic per wave).
__global__ void __launch_bounds__(256) k_march_static_trip(PnTrip* trip, const int* __restrict__ rays_alive, const float* __restrict__ rays_t,
                                                           const float* __restrict__ rays_o, const float* __restrict__ rays_d, float bound,
                                                           float dt_gamma, uint32_t max_steps, uint32_t C, uint32_t H,
                                                           const uint8_t* __restrict__ grid, const float* __restrict__ fars, float* __restrict__ xyzs,
                                                           float* __restrict__ dirs, float* __restrict__ deltas, int* __restrict__ list) {
    const uint32_t n_alive = (uint32_t)trip->n_alive, n_step = (uint32_t)trip->n_step;
    const int lane = threadIdx.x & 63;
    for (uint32_t chunk = blockIdx.x; chunk * 256u < n_alive; chunk += gridDim.x) {
        const uint32_t n = chunk * 256u + threadIdx.x;
        const uint32_t emitted = n < n_alive ? march_static_one<false, true>(n, n_step, rays_alive, rays_t, rays_o, rays_d, bound, dt_gamma, max_steps, C, H, grid,
                                                                             fars, xyzs, dirs, deltas, nullptr)
                                             : 0u;
        int inc = (int)emitted;  // inclusive wave scan of the sample counts, one atomic per wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_up(inc, o);
            if (lane >= o) inc += u;
        }
        const int total = __shfl(inc, 63);
        int base = 0;
        if (lane == 63 && total > 0) base = atomicAdd(&trip->n_samples, total);
        base = __shfl(base, 63);
        const int first = base + inc - (int)emitted;
        for (uint32_t s = 0; s < emitted; s++) list[first + s] = (int)(n * n_step + s);
    }
}
