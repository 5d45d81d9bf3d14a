// The frame workspace (pn_frame) and the frame driver's own kernels: k_frame_tables, k_frame_prologue, k_frame_finish and the one-lane helpers.
// Part of the render unit (included by pn_render_ops.hip only, behind the trip kernels).
#pragma once
#include <float.h>

#include "pn_cell_hash.h"
#include "pn_compact.h"
#include "pn_march_kernels.h"
#include "pn_near_far.h"
#include "pn_side_tables.h"

#define PN_MAX_TRIPS 1100
#define PN_MIN_RAY_BATCH 64  // smallest pn_render_opts::ray_batch (sizes the group records of a workspace)
#define PN_TRIP_BATCH 8
#define PN_TRIP_MARGIN 2  // trips a captured render carries beyond what its sizing frame needed (harness: measured + 2)
#define PN_TIMED_TRIPS 64

#include "pn_trips_fused.h"

struct pn_frame {
    uint32_t max_rays, max_vtx, max_cells;
    float *nears, *fars, *rays_t, *xyzs, *dirs, *deltas, *sigmas, *rgbs;
    float* acc_image;  // [max_rays,3] colour accumulated by composite; the epilogue writes image = acc + (1 - weights_sum) * bg, so a frame can be
                       // continued with more trips and finished again (pn_render_continue)
    int *alive_a, *alive_b, *list, *chunk_counts;
    TailEntry* tail;    // [PN_SEGS x seg_cap] rays handed from k_march to k_march_tail
    int* list_seg;      // [PN_SEGS x seg_cap] segmented sample list of a list trip (k_list_pack -> list)
    int* active_seg;    // [PN_SEGS x seg_cap] trip 0: the slots k_march_skip left something to march for
    uint32_t seg_cap;
    uint32_t* cell_bits;  // [2][(max_cells + 31) / 32] bit c: search cell c has candidates / is within one cell of such a cell (cleared by
                          // k_frame_tables, set by k_frame_prologue: frame_lists_block)
    uint32_t* grid_regions;  // [PN_GRID_REGION_WORDS] --cut frames: the region map of the skip pre-pass (MarchIO::grid_regions; k_frame_prologue)
    float* fars_eff;      // [max_rays] the rays' ends shortened to where they can still find candidates (k_march_skip)
    int* seg_counters;  // [6][PN_SEGS] counters, one per 128 B: tail | sample | emitted | tail cursor | tail back (cleared by each trip's compaction) | active (k_frame_prologue: frame_rays_block)
    int* tail_counts;   // [PN_MAX_TRIPS + 2] diagnostics: rays each trip handed to the tail pass
    int *pig_cnt, *pig_bgn, *pig_idx, *pig_cursor;
    MarchSide side;  // candidate lists + packed IP records of the cooperative march
    PnTrip* trips;  // [PN_MAX_TRIPS + 2]
    PnGroup* groups;     // [2][max_groups] ray-group records of the current / next trip (trip parity), see PnGroup
    int* group_cnt;      // [max_groups] survivors per group (composite -> trip_epilogue, which clears them)
    uint32_t max_groups;
    PnFrameDev* dev;
    float* cut_bounds;
    PnTrip* trips_pinned;  // host-pinned mirror
    PnFrameDev* dev_pinned;
    float cut_bounds_host[6];
    int cut_bounds_valid;
    int last_trips;  // trips enqueued by the last render (incl. continuations)
    uint32_t last_N;
    uint32_t last_group_rays;  // ray_batch of the last render (a continuation must use the same)
    int tables_n_vtx;  // IP count the workspace's tables were built for (0: none); pn_render_opts::reuse_tables
    unsigned long long* march_counters;  // device [4], see MarchParams::stats
    int march_counters_on;
    hipEvent_t ev[PN_TIMED_TRIPS][3];    // measurement mode: before march / after march / after network, per trip
    int timed_trips;
    unsigned long long* stamps;          // device [PN_TIMED_TRIPS][3]: the same three points as 100 MHz wall-clock stamps written by one-lane kernels
    int stamped;                         // — the form that also works inside a captured graph (HIP events recorded in a graph cannot be timed)
    // the fused later trips (pn_trips_fused.h)
    int* fused_ctl;                      // [PN_FUSED_CTL_INTS] hand-out cursors, per-trip counters, workgroups done: zero between launches
    uint32_t fused_blocks;               // workgroups of a fused launch (one per CU); xyzs / dirs / deltas / sigmas / rgbs hold 64 slots per wave of it
    unsigned long long* fused_clocks;    // device [8] phase clocks of the fused launches (march_counters_on & 4)
    int fused_first;                     // first trip the last render ran fused (-1: none): where its time stamps sit
    float* t_resume;                     // [max_rays] per alive slot of a frame's first trip: where k_march_skip left the ray
    int* blist;                          // whole-frame fused launch: [2 x blist_cap] ray ids of the first trip's shares / of the rays that outlive it
    int4* strag;                         // [blist_cap] its rays still searching after the one-lane rounds
    uint32_t blist_cap;
    int skip_done;                       // the last render on this workspace ran k_march_skip (a continuation from trip 0 must not run it again)
    int head_marched;                    // ... and the first trip's march launches (pn_render_opts.fused_fold): a continuation from trip 0 goes on behind them
    int fused_mode;                      // form of the last fused launch that was enqueued: 0 later trips, 1 whole frame, 2 first trip folded in (pn_trips_fused.h)
};

__global__ void k_set_aabb(PnFrameDev* dev, float a0, float a1, float a2, float a3, float a4, float a5) {
    dev->aabb[0] = a0; dev->aabb[1] = a1; dev->aabb[2] = a2; dev->aabb[3] = a3; dev->aabb[4] = a4; dev->aabb[5] = a5;
    dev->resolution[0] = dev->resolution[1] = dev->resolution[2] = dev->resolution[3] = 0;
    dev->err = 0;
}

__global__ void k_reset_unfinished(PnFrameDev* dev) { dev->unfinished = 0; }

// image = acc + (1 - weights_sum) * bg ; depth = clamp(depth - nears, 0) / (fars - nears) (renderer.py:896-899)
// The first wave of the launch also closes the frame's books: trips_run (+ the trips a fused launch ran, whose number only the device knows), the summary
// of the trip records (what pn_render_status reports) and the rays a fixed-trip render left alive.  count_left (the static render): alive_at_exit also
// counts the rays max_steps ended the loop on (PnTrip::n_left), as the op-by-op loop run_cuda_ops reports them; more trips do nothing for those, so they
// are not `unfinished`.  (The deformed frame's fused launch does not know that count, so none of the deformed forms reports it.)
__global__ void __launch_bounds__(256) k_frame_finish(uint32_t N, float bg, const float* __restrict__ nears, const float* __restrict__ fars,
                                                      const float* __restrict__ weights_sum, const float* __restrict__ depth_0,
                                                      const float* __restrict__ acc, float* __restrict__ image, float* __restrict__ depth,
                                                      const PnTrip* __restrict__ trips, PnFrameDev* dev, int trips_run, int add_fused, int count_left) {
    const uint32_t i = threadIdx.x + blockIdx.x * blockDim.x;
    if (i < 64) {
        const int lane = (int)i;
        const int t_final = min(trips_run + (add_fused ? dev->fused_trips : 0), PN_MAX_TRIPS);
        int n_trips = 0;
        long long n_samples = 0;
        for (int k = lane; k < t_final; k += 64) {
            const PnTrip* r = trips + k;
            if (r->n_alive > 0) n_trips++;
            n_samples += r->dense ? r->n_emitted : r->n_samples;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { n_trips += __shfl_xor(n_trips, o); n_samples += __shfl_xor(n_samples, o); }
        if (lane == 0) {
            const int left = trips[t_final].n_alive;
            dev->trips_run = t_final;
            dev->fused_trips = 0;
            dev->stat_trips = n_trips;
            dev->stat_samples = n_samples;
            dev->alive_at_exit = left + (count_left ? trips[t_final].n_left : 0);
            if (left > 0) atomicAdd(&dev->unfinished, left);
        }
    }
    if (i >= N) return;
    const float k = (1 - weights_sum[i]) * bg;
    image[i * 3] = acc[i * 3] + k;
    image[i * 3 + 1] = acc[i * 3 + 1] + k;
    image[i * 3 + 2] = acc[i * 3 + 2] + k;
    depth[i] = fmaxf(depth_0[i] - nears[i], 0.0f) / (fars[i] - nears[i]);
}

// measurement: a stream-ordered time stamp (constant 100 MHz clock) as an ordinary kernel node, so that it can live inside a captured graph
__global__ void k_stamp(unsigned long long* slot) { *slot = __builtin_amdgcn_s_memrealtime(); }

// ---- fused frame prologue (3 launches instead of 13; every one of them was a few-microsecond kernel with a launch gap)
// (1) k_frame_tables, ONE workgroup of 1024 threads: IP bounding box +-1e-3 and spatial-hash resolution (nerf/renderer.py:782-791), the spatial
//     hash itself (count -> scan -> cursor fill -> per-cell sort, = k_pig_*) and the per-cell candidate-list offsets (k_nb_count
//     + scan).  The phases talk through global memory (L2) with relaxed agent-scope atomic loads where a value was produced by
//     an atomic or by another thread of the block, and __syncthreads() in between.
//     LARGE = false: everything in this one workgroup, per-cell counters in LDS (two 16-bit counters per word: up to ~290 k cells minus the
//     staged index table fit the 160 KB).  LARGE = true: the grid is too large for that (bound 2 with --cut: the spatial hash spans +-bound,
//     67^3 = 300 k cells at hgs 0.06) — this kernel only does the bounding box / resolution part and the tables are built by the
//     multi-workgroup kernels of get_pnts_in_grids (k_pig_*) + k_nb_count + a second scan; same tables, bit for bit.
template <bool LARGE>
__global__ void __launch_bounds__(1024) k_frame_tables(const float* __restrict__ p_def, int n_vtx, int cut, float bound, float hgs, int max_cells,
                                                       PnFrameDev* dev, int* pig_cnt, int* pig_bgn, int* pig_idx, int* pig_cursor, uint32_t* cell_bits) {
    extern __shared__ unsigned cnt2[];  // per-cell point counts, two 16-bit counters per word (a cell never holds 65 536 IPs)
    for (int w = threadIdx.x; w < 2 * ((max_cells + 31) / 32); w += blockDim.x) cell_bits[w] = 0u;  // both maps; set by k_frame_prologue (frame_lists_block)
    __shared__ float smin[3][16], smax[3][16];
    __shared__ float sh_min[3];
    __shared__ int sh_res[4];
    __shared__ int wsum[16];
    __shared__ int carry_s;
    float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    for (int i = threadIdx.x; i < n_vtx; i += blockDim.x)
#pragma unroll
        for (int c = 0; c < 3; c++) { const float v = p_def[i * 3 + c]; mn[c] = fminf(mn[c], v); mx[c] = fmaxf(mx[c], v); }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < 3; c++) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { mn[c] = fminf(mn[c], __shfl_xor(mn[c], o)); mx[c] = fmaxf(mx[c], __shfl_xor(mx[c], o)); }
        if (lane == 0) { smin[c][wid] = mn[c]; smax[c][wid] = mx[c]; }
    }
    __syncthreads();
    if (threadIdx.x == 0) {  // renderer.py:782-791
        int ncell = 1;
        for (int c = 0; c < 3; c++) {
            float a = smin[c][0], b = smax[c][0];
            for (int w = 1; w < 16; w++) { a = fminf(a, smin[c][w]); b = fmaxf(b, smax[c][w]); }
            if (cut) { a = -bound; b = bound; }
            const float lo = a - 1e-3f, hi = b + 1e-3f;
            dev->aabb[c] = lo;
            dev->aabb[3 + c] = hi;
            sh_min[c] = lo;
            const int r = (int)ceilf((hi - lo) / hgs);
            dev->resolution[c] = r;
            sh_res[c] = r;
            ncell *= r;

        }
        int err = 0;
        if (ncell > max_cells || ncell <= 0) { err = 4; ncell = 0; }
        dev->resolution[3] = ncell;
        dev->err = err;
        dev->nb_alloc = 0;
        sh_res[3] = ncell;
        carry_s = 0;
    }
    __syncthreads();
    const int n_grid_all = sh_res[3], r0 = sh_res[0], r1 = sh_res[1], r2 = sh_res[2];
    const float b0 = sh_min[0], b1 = sh_min[1], b2 = sh_min[2];
    if (n_grid_all == 0) return;
    // the cells that hold integration points, exactly as p2g files them (a point outside the grid whose flat index still lies in [0, n_grid) is filed under that
    // index, as in the reference): their extent per axis -> PnFrameDev::ip_lo / ip_hi (k_frame_prologue builds lists only near them)
    __shared__ int s_lo[3], s_hi[3];
    if (threadIdx.x < 3) { s_lo[threadIdx.x] = 0x7fffffff; s_hi[threadIdx.x] = -1; }
    __syncthreads();
    // (in registers and by wave shuffles first, like the bounding box above, then one atomic pair per wave and axis: six atomics per point on three shared
    // words were ~62 k same-address LDS atomics from this ONE workgroup on every frame's chain)
    int c_lo[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, c_hi[3] = {-1, -1, -1};
    for (int p = threadIdx.x; p < n_vtx; p += blockDim.x) {
        const int q0 = (int)floorf((p_def[p * 3] - b0) / hgs), q1 = (int)floorf((p_def[p * 3 + 1] - b1) / hgs), q2 = (int)floorf((p_def[p * 3 + 2] - b2) / hgs);
        const int gid = q2 * r1 * r0 + q1 * r0 + q0;
        if (gid < 0 || gid >= n_grid_all) continue;
        const int cc[3] = {gid % r0, (gid / r0) % r1, gid / (r0 * r1)};
#pragma unroll
        for (int c = 0; c < 3; c++) { c_lo[c] = min(c_lo[c], cc[c]); c_hi[c] = max(c_hi[c], cc[c]); }
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { c_lo[c] = min(c_lo[c], __shfl_xor(c_lo[c], o)); c_hi[c] = max(c_hi[c], __shfl_xor(c_hi[c], o)); }
        if (lane == 0) { atomicMin(&s_lo[c], c_lo[c]); atomicMax(&s_hi[c], c_hi[c]); }
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const bool any = s_hi[threadIdx.x] >= 0;
        dev->ip_lo[threadIdx.x] = any ? s_lo[threadIdx.x] : 0;
        dev->ip_hi[threadIdx.x] = any ? s_hi[threadIdx.x] : -1;
    }
    if (LARGE) return;  // the tables themselves are built by the multi-workgroup kernels (pn_frame_prologue)
    const int n_grid = n_grid_all;
    for (int g = threadIdx.x; g < (n_grid + 1) / 2; g += blockDim.x) cnt2[g] = 0u;
    __syncthreads();
    auto cell_of = [&](int p) {  // p2g, nerf/utils.py:389-407
        const int g0 = (int)floorf((p_def[p * 3] - b0) / hgs);
        const int g1 = (int)floorf((p_def[p * 3 + 1] - b1) / hgs);
        const int g2 = (int)floorf((p_def[p * 3 + 2] - b2) / hgs);
        const int gid = g2 * r1 * r0 + g1 * r0 + g0;
        return (gid < 0 || gid >= n_grid) ? -1 : gid;
    };
    auto count_of = [&](int g) { return (int)((cnt2[g >> 1] >> (16 * (g & 1))) & 0xFFFFu); };
    for (int p = threadIdx.x; p < n_vtx; p += blockDim.x) {
        const int gid = cell_of(p);
        if (gid >= 0) atomicAdd(&cnt2[gid >> 1], 1u << (16 * (gid & 1)));
        else atomicOr(&dev->err, 2);
    }
    __syncthreads();
    // exclusive scan of the counts -> pig_cnt / pig_bgn / pig_cursor.  (Rounds 1-2 also summed every cell's 27-neighbourhood here and scanned
    // that for the candidate-list offsets: 27 LDS reads + the neighbour arithmetic per cell on ONE compute unit were 50 of this kernel's 82 us.
    // The lists now get their space from a bump counter in k_frame_prologue, which runs on the whole chip.)
    {
        int* out_cnt = pig_cnt;
        int* out_bgn = pig_bgn;
        int* out_cur = pig_cursor;
        for (int base = 0; base < n_grid; base += 4096) {
            const int i0 = base + threadIdx.x * 4;
            int v[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int c = i0 + k;
                int val = 0;
                if (c < n_grid) {
                    val = count_of(c);
                    out_cnt[c] = val;
                }
                v[k] = val;
            }
            const int tsum = v[0] + v[1] + v[2] + v[3];
            int inc = tsum;  // inclusive wave scan
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int u = __shfl_up(inc, o);
                if (lane >= o) inc += u;
            }
            if (lane == 63) wsum[wid] = inc;
            __syncthreads();
            int woff = 0;
            for (int w = 0; w < wid; w++) woff += wsum[w];
            int total = 0;
            for (int w = 0; w < 16; w++) total += wsum[w];
            int run = carry_s + woff + inc - tsum;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (i0 + k < n_grid) { out_bgn[i0 + k] = run; out_cur[i0 + k] = run; }
                run += v[k];
            }
            __syncthreads();
            if (threadIdx.x == 0) carry_s += total;
            __syncthreads();
        }
        if (threadIdx.x == 0) carry_s = 0;
        __syncthreads();
    }
    // cursor fill (get_pig_idx, nerf/utils.py:427-443): slots claimed through the per-cell cursor, entries staged in LDS ...
    int* lidx = reinterpret_cast<int*>(cnt2 + (max_cells + 1) / 2);
    for (int p = threadIdx.x; p < n_vtx; p += blockDim.x) {
        const int gid = cell_of(p);
        if (gid >= 0) lidx[atomicAdd(pig_cursor + gid, 1)] = p;
    }
    __syncthreads();
    // ... then ascending point id inside each cell (k_pig_sort): the table does not depend on the order of the atomics
    for (int g = threadIdx.x; g < n_grid; g += blockDim.x) {
        const int c = count_of(g);
        if (c < 2) continue;
        int* a = lidx + __hip_atomic_load(pig_bgn + g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        for (int i = 1; i < c; i++) {
            const int v = a[i];
            int j = i - 1;
            while (j >= 0 && a[j] > v) { a[j + 1] = a[j]; j--; }
            a[j + 1] = v;
        }
    }
    __syncthreads();
    for (int p = threadIdx.x; p < n_vtx; p += blockDim.x) pig_idx[p] = lidx[p];
}

// (2) k_frame_prologue, ONE launch for everything else the frame needs before its first trip, three independent block ranges:
//     [0, list_blocks)  candidate lists, 8 lanes per cell and 32 cells per workgroup round: the 27 neighbours' counts (lane j holds visiting
//                       positions j, j+8, j+16, j+24), their running sum inside the 8-lane group (= where each neighbour's entries go), list space
//                       by ONE returning atomic per workgroup round on dev->nb_alloc (the order of the lists in memory means nothing; an
//                       atomic per cell on one address would serialise, see PN_SEGS), the entries, the (begin, end) record, and the two cell maps:
//                       "has candidates" and — scattered to the 27 neighbours of every such cell — "within one cell of a cell with candidates".
//                       The maps are a few cache lines (chair: 10 k cells = 10 lines) and atomics on one LINE queue like atomics on one address
//                       (measured: 160 k atomicOr straight to global memory made this kernel 125 us), so every workgroup collects its bits in
//                       LDS (lds_words > 0) and ORs only its non-zero words into the global maps;
//     [.., + pack_blocks)  the packed IP records (k_pack_ip);
//     the rest             near / far (pn_near_far.h) + the per-ray initialisation: zeroed accumulators (renderer.py:807-809), rays_alive = arange(N) (:828),
//                          rays_t = nears (:829), zeroed trip records / counters, trip 0 = (N rays, n_step 1).  Needs only the bounding box.
struct FramePrologue {
    // lists
    int n_grid_max; const int* n_grid_dev; const int* res; const int* pig_cnt; const int* pig_bgn; const int* pig_idx; const float* p_def; int swap;
    int2* nb_rng; float4* nb; int nb_capacity; int list_blocks; uint32_t* cell_bits; int lds_words;
    // records
    int pack_blocks; int n_vtx; const float* p_ori; const float* F_IP; const float* dF_IP; float* rec;
    // rays
    const float* rays_o; const float* rays_d; PnFrameDev* dev; uint32_t N; float min_near; float* nears; float* fars; float* rays_t; PnTrip* trips;
    int* tail_counts; int* seg_counters; int n_trip_records; int* alive; float* weights_sum; float* depth_0; float* image; PnGroup* groups;
    int* group_cnt; uint32_t group_rays; uint32_t n_groups; int* chunk_words;
    uint32_t tile_w, tile_lw;  // tile_w > 0: alive list starts in 16 x 4 pixel tile order (pn_render_opts.ray_tile_w, validated by the host)
    // early_finish: the frame's epilogue is left to the fused launch (pn_trips_fused.h: finalize) — every ray gets the pixel of a ray without samples here
    int early_finish; float bg; float* image_out; float* depth_out;
    // --cut frames: the region map (MarchIO::grid_regions): gr_blocks workgroups, a lane per region of the (H / 8)^3 grid
    const uint8_t* grid; uint32_t* grid_regions; int gr_blocks; int gr_R; int gr_C; uint32_t gr_H; float gr_bound; const float* cut_bounds;
};
#define PN_GRID_REGION_WORDS 1024  // 32 768 regions: H <= 256

__device__ __forceinline__ void frame_lists_block(const FramePrologue& a) {
    extern __shared__ uint32_t lds_bits[];  // [2][lds_words] when lds_words > 0
    __shared__ int wtot[4];
    __shared__ int blk_base;
    const int n_grid = min(*a.n_grid_dev, a.n_grid_max);
    const int r0 = a.res[0], r1 = a.res[1], r2 = a.res[2];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, sub = threadIdx.x & 7;
    const int words = (a.n_grid_max + 31) / 32;
    const int per_round = a.list_blocks * 32;
    const int ilo0 = a.dev->ip_lo[0], ilo1 = a.dev->ip_lo[1], ilo2 = a.dev->ip_lo[2], ihi0 = a.dev->ip_hi[0], ihi1 = a.dev->ip_hi[1], ihi2 = a.dev->ip_hi[2];
    const bool in_lds = a.lds_words > 0;
    if (in_lds) {
        for (int w = threadIdx.x; w < 2 * a.lds_words; w += blockDim.x) lds_bits[w] = 0u;
        __syncthreads();
    }
    for (int c0 = 0; c0 < n_grid; c0 += per_round) {  // uniform trip count: the round's workgroup-wide sum needs every thread
        const int c = c0 + (int)blockIdx.x * 32 + ((int)threadIdx.x >> 3);
        const bool valid = c < n_grid;
        int g0 = 0, g1 = 0, g2 = 0;
        if (valid) nb_cell_coords(c, r0, r1, g0, g1, g2);
        // a cell more than one cell away from every integration point has an empty list: no neighbour to look at (PnFrameDev::ip_lo / ip_hi)
        const bool near_ips = valid && g0 >= ilo0 - 1 && g0 <= ihi0 + 1 && g1 >= ilo1 - 1 && g1 <= ihi1 + 1 && g2 >= ilo2 - 1 && g2 <= ihi2 + 1;
        int cell[4], cnt[4], before[4];
        int total = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {  // visiting position q = 0 is the cell itself, q = 1..26 its neighbours q - 1
            const int q = sub + 8 * k;
            cell[k] = (near_ips && q < 27) ? ((q == 0) ? c : nb_neighbour(q - 1, a.swap, g0, g1, g2, r0, r1, r2)) : -1;
            cnt[k] = cell[k] >= 0 ? a.pig_cnt[cell[k]] : 0;
            int inc = cnt[k];  // running sum over the 8 lanes of the group
#pragma unroll
            for (int o = 1; o < 8; o <<= 1) {
                const int u = __shfl_up(inc, o, 8);
                if (sub >= o) inc += u;
            }
            before[k] = total + inc - cnt[k];
            total += __shfl(inc, 7, 8);
        }
        // list space: exclusive sum of the round's 32 totals + one bump of the frame's counter
        const int mine = (sub == 0) ? total : 0;
        int inc = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_up(inc, o);
            if (lane >= o) inc += u;
        }
        if (lane == 63) wtot[wid] = inc;
        const int in_wave = __shfl(inc - mine, lane & ~7);  // the group's first lane holds the cell's exclusive offset
        __syncthreads();
        if (threadIdx.x == 0) {
            const int sum = wtot[0] + wtot[1] + wtot[2] + wtot[3];
            blk_base = sum ? atomicAdd(&a.dev->nb_alloc, sum) : 0;
        }
        __syncthreads();
        int w0 = blk_base + in_wave;
        for (int w = 0; w < wid; w++) w0 += wtot[w];
        __syncthreads();  // wtot / blk_base are rewritten by the next round
        if (!valid) continue;
        const bool fits = w0 + total <= a.nb_capacity;
        if (sub == 0) {
            a.nb_rng[c] = (total > 0 && fits) ? make_int2(w0, w0 + total) : make_int2(0, 0);
            if (total > 0 && !fits) atomicOr(&a.dev->err, 8);
        }
        if (total == 0 || !fits) continue;
        if (sub == 0) atomicOr((in_lds ? lds_bits : a.cell_bits) + (c >> 5), 1u << (c & 31));
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (cell[k] < 0) continue;
            // second map: `cell[k]` lies within one cell of a cell with candidates
            atomicOr((in_lds ? lds_bits + a.lds_words : a.cell_bits + words) + (cell[k] >> 5), 1u << (cell[k] & 31));
            const int n = cnt[k], b = a.pig_bgn[cell[k]];
            for (int i = 0; i < n; i++) {
                const int ip = a.pig_idx[b + i];
                a.nb[w0 + before[k] + i] = make_float4(a.p_def[ip * 3], a.p_def[ip * 3 + 1], a.p_def[ip * 3 + 2], __int_as_float(ip));
            }
        }
    }
    if (in_lds) {
        __syncthreads();
        for (int w = threadIdx.x; w < 2 * a.lds_words; w += blockDim.x) {
            const uint32_t v = lds_bits[w];
            if (v) atomicOr(a.cell_bits + (w < a.lds_words ? w : words + (w - a.lds_words)), v);
        }
    }
}

__device__ __forceinline__ void frame_rays_block(const FramePrologue& a, uint32_t block) {
    const uint32_t n = threadIdx.x + block * blockDim.x;
    if (block == 0 && a.groups) {  // trip 0 of every group: all its rays, one sample each (max(min(N_b // N_b, 8), 1))
        for (uint32_t b = threadIdx.x; b < a.n_groups; b += blockDim.x) {
            a.groups[b] = PnGroup{(int)(b * a.group_rays), 1, (int)(b * a.group_rays), 0};
            a.group_cnt[b] = 0;
        }
    }
    // the trip records (1102 x 256 B) are cleared four to a workgroup, one dword per lane (one workgroup clearing all of them was this launch's
    // critical path); trip 0 (n_step == 1) is a list trip over all N rays
    {
        const int t = (int)block * 4 + (int)(threadIdx.x >> 6), w = threadIdx.x & 63;
        if (t < a.n_trip_records) {
            int v = 0;
            if (t == 0 && w == 0) v = (a.dev->err & 7) ? 0 : (int)a.N;  // flags of k_frame_tables stop the frame
            if (t == 0 && w == 1) v = 1;                                // n_step = max(min(N // N, 8), 1)
            reinterpret_cast<int*>(a.trips + t)[w] = v;
            if (w == 0) a.tail_counts[t] = 0;
        }
        // a frame with fewer rays than that: the last workgroup clears what is left
        if (block + 1 == gridDim.x - (uint32_t)(a.list_blocks + a.pack_blocks)) {
            for (int t2 = ((int)block + 1) * 4 + (int)(threadIdx.x >> 6); t2 < a.n_trip_records; t2 += 4) {
                reinterpret_cast<int*>(a.trips + t2)[w] = 0;
                if (w == 0) a.tail_counts[t2] = 0;
            }
        }
    }
    if (block == 0)
        for (int t = threadIdx.x; t < 6 * PN_SEGS; t += blockDim.x) a.seg_counters[t * PN_SEG_STRIDE] = 0;
    if (block == 0 && threadIdx.x == 0) {
        // Every frame starts with no fused trips on its books: a frame finished INSIDE a fused launch leaves its count behind (no k_frame_finish ran to
        // clear it), and a later frame on this pn_frame whose fused launch steps aside would otherwise read it as "ran to the end" (round-4 advisor).
        a.dev->fused_trips = 0;
        if (a.early_finish) {  // the frame's books until the fused launch closes them (if it steps aside: an unfinished frame at trip 0)
            a.dev->trips_run = 0; a.dev->stat_trips = 0; a.dev->stat_samples = 0; a.dev->alive_at_exit = (int)a.N;
        }
    }
    if (threadIdx.x == 0) a.chunk_words[block] = 0;  // one (tag, count) word per 256 rays (+ the spare ones by the last workgroup), see k_composite_compact
    if (threadIdx.x < 2 && block + 1 == gridDim.x - (uint32_t)(a.list_blocks + a.pack_blocks)) a.chunk_words[block + 1 + threadIdx.x] = 0;
    if (n >= a.N) return;
    const float* aabb = a.dev->aabb;
    const float ox = a.rays_o[n * 3], oy = a.rays_o[n * 3 + 1], oz = a.rays_o[n * 3 + 2];
    const float dx = a.rays_d[n * 3], dy = a.rays_d[n * 3 + 1], dz = a.rays_d[n * 3 + 2];
    float near, far;
    pn_near_far(aabb, ox, oy, oz, dx, dy, dz, a.min_near, near, far);  // pn_near_far.h, shared with the stand-alone op
    a.nears[n] = near;
    a.fars[n] = far;
    a.rays_t[n] = near;  // rays_t = nears.clone() (renderer.py:829)
    // rays_alive = arange(N) (renderer.py:828) — or, for a whole image, the same set in 16 x 4 pixel tiles: slot n = pixel (n & 15, (n >> 4) & 3) of
    // tile n / 64 (tiles row-major).  A wave's 64 slots are then a tile, and every later alive list (stable compaction) keeps that order
    uint32_t ray = n;
    if (a.tile_w) {
        const uint32_t lw = a.tile_lw, tile = n >> 6, in = n & 63u, tiles_x = a.tile_w >> lw;  // tile of (1 << lw) x (64 >> lw) pixels, lw = 4
        ray = ((tile / tiles_x) * (64u >> lw) + (in >> lw)) * a.tile_w + ((tile % tiles_x) << lw) + (in & ((1u << lw) - 1u));
    }
    a.alive[n] = (int)ray;
    a.weights_sum[n] = 0.f;
    a.depth_0[n] = 0.f;
    a.image[n * 3] = 0.f; a.image[n * 3 + 1] = 0.f; a.image[n * 3 + 2] = 0.f;
    if (a.early_finish) {  // k_frame_finish's expressions for weights_sum = depth_0 = acc = 0 (renderer.py:896-899)
        const float k = (1 - 0.f) * a.bg;
        a.image_out[n * 3] = 0.f + k; a.image_out[n * 3 + 1] = 0.f + k; a.image_out[n * 3 + 2] = 0.f + k;
        a.depth_out[n] = fmaxf(0.f - near, 0.0f) / (far - near);
    }
}

__global__ void __launch_bounds__(256) k_frame_prologue(FramePrologue a) {
    const int b = (int)blockIdx.x;
    if (b < a.list_blocks) { frame_lists_block(a); return; }
    if (b < a.list_blocks + a.pack_blocks) {  // k_pack_ip
        const int t = threadIdx.x + (b - a.list_blocks) * 256;
        const int ip = t / PN_REC_FLOATS, j = t % PN_REC_FLOATS;
        if (ip < a.n_vtx) a.rec[t] = pnm2::pack_ip_float(j, ip, a.p_ori, a.p_def, a.F_IP, a.dF_IP);
        return;
    }
    if (b < a.list_blocks + a.pack_blocks + a.gr_blocks) {  // region map of the density bitfield (pn_march_skip.h: region_dda)
        const int R = a.gr_R, n_reg = R * R * R;
        const int r = threadIdx.x + (b - a.list_blocks - a.pack_blocks) * 256;
        if (r < n_reg) {
            bool any = false;
            const int b0 = r % R, b1 = (r / R) % R, b2 = r / (R * R);
            // a region is V = (H / R)^3 voxels = V / 64 consecutive 8-byte words of a level's bitfield in morton order (R = H / 8: a 64-byte line; R = H / 4: one word)
            const uint32_t vox_side = a.gr_H / (uint32_t)R, words_per_region = (vox_side * vox_side * vox_side) >> 6;
            const uint32_t words_per_level = (a.gr_H * a.gr_H * a.gr_H) >> 6;
            const uint2* g2 = reinterpret_cast<const uint2*>(a.grid);
            uint32_t acc_l[3] = {0u, 0u, 0u};   // occupancy of the region on level l (gr_C <= 3)
            for (int l = 0; l < a.gr_C; l++) {
                // on level l (R blocks over +-2^l) the region is the aligned cube of 2^j blocks per axis at R / 2 + (b - R / 2) 2^j, j = C - 1 - l — contiguous
                // words in morton order — or lies outside the level's volume, where no point can be tested on it
                const int j = a.gr_C - 1 - l, side = 1 << j;
                const int c0 = R / 2 + (b0 - R / 2) * side, c1 = R / 2 + (b1 - R / 2) * side, c2 = R / 2 + (b2 - R / 2) * side;
                if (c0 < 0 || c1 < 0 || c2 < 0 || c0 + side > R || c1 + side > R || c2 + side > R) continue;
                const uint32_t first = (uint32_t)l * words_per_level + pnm2::morton3D((uint32_t)c0, (uint32_t)c1, (uint32_t)c2) * words_per_region;
                const uint32_t n_words = words_per_region << (3 * j);
                for (uint32_t q = 0; q < n_words; q++) {
                    const uint2 v = g2[(size_t)first + q];
                    acc_l[l] |= v.x | v.y;
                }
            }
            // map L serves the rays whose mip level cannot fall below L any more (level >= mip_from_dt(dt), dt grows with t): occupied on a level >= L
            for (int L = a.gr_C - 2; L >= 0; L--) acc_l[L] |= acc_l[L + 1];
            // ... or it meets the cut box: x in (cb0, cb1), y > cb2, z in (cb4, cb5) — a superset of the reference's test (raymarching.cu:1210 compares x with
            // cut_bounds[3] where y is meant), widened by a hundredth of a region
            const float w = 2.0f * a.gr_bound / (float)R, eps = 0.01f * w;
            const float x0 = -a.gr_bound + (float)b0 * w, y0 = -a.gr_bound + (float)b1 * w, z0 = -a.gr_bound + (float)b2 * w;
            const float* cb = a.cut_bounds;
            if (x0 + w > cb[0] - eps && x0 < cb[1] + eps && y0 + w > cb[2] - eps && z0 + w > cb[4] - eps && z0 < cb[5] + eps) any = true;
            for (int L = 0; L < a.gr_C; L++) {   // one map per minimum level, behind each other
                const unsigned long long m = __ballot(any || acc_l[L] != 0u);
                if ((threadIdx.x & 63) == 0) {   // (R^3 is a multiple of 64: whole words only, whole waves inside n_reg)
                    a.grid_regions[(size_t)L * (n_reg >> 5) + (r >> 5)] = (uint32_t)m;
                    a.grid_regions[(size_t)L * (n_reg >> 5) + (r >> 5) + 1] = (uint32_t)(m >> 32);
                }
            }
        }
        return;
    }
    frame_rays_block(a, (uint32_t)(b - a.list_blocks - a.pack_blocks - a.gr_blocks));
}
